"""What tests/_select_perceiver.py promises, checked without a GPU: every draw of tests/test_perceiver_exact_gpu.py meets its
conditions (the gap need_gap(t_x + n), bf16-integer operands, n distinct keys per (sample, head) with key 0, the last x key, the first
and the last latent key and the first key of the x segment's ragged 16-key tile among them); the CPU emulation of the arithmetic
include/minsdtf_hip_resampler.h pins returns the expected bits on every draw; and every fault of a two-segment kernel - the wrong
segment, the wrong head, the wrong sample, an off-by-one at the segment boundary - applied INSIDE that emulation is refused by the
exact comparison."""
import pytest
import torch

import _select as S
import _select_perceiver as SP

BF16 = torch.bfloat16
IDS = [SP.run_id(*r) for r in SP.RUNS]


def _refused(fn):
    try:
        fn()
    except AssertionError as e:
        return str(e)
    return None


@pytest.mark.parametrize("run", SP.RUNS, ids=IDS)
def test_conditions_hold_for_every_case(run):
    p = SP.problem(*run)
    G = SP.conditions(p)
    assert G >= S.need_gap(p.t_x + p.n) and float(p.q.abs().max()) <= 8 and float(p.k.abs().max()) <= 8
    B, H, n, t, _sl2 = run
    assert tuple(p.q.shape) == (B, n, H * 64) and tuple(p.k.shape) == tuple(p.v.shape) == (B, t + n, H * 64)
    kx, vx, kl, vl = SP.segments(p)
    assert kx.shape[1] == vx.shape[1] == t and kl.shape[1] == vl.shape[1] == n


def test_forced_keys_name_both_segments_and_the_ragged_tile():
    assert SP.forced(257, 16) == [0, 256, 257, 272] and SP.forced(77, 5) == [0, 64, 76, 77, 81]
    assert SP.forced(1, 3) == [0, 1, 3] and SP.forced(64, 16) == [0, 63, 64, 79] and SP.forced(40, 9) == [0, 32, 39, 40, 48]
    for _B, _H, n, t in SP.SHAPES:
        assert len(SP.forced(t, n)) <= n


def test_conditions_refuse_a_draw_that_breaks_them():
    run = (1, 2, 5, 77, 1.0)
    SP.conditions(SP.problem(*run))

    def fresh():
        SP._DRAWS.clear()
        return SP.problem(*run)

    p = fresh()
    match = int(p.pi[0, 0, 0])                                        # a key that no query selects comes within one bit of a match
    near = next(j for j in range(1, 76) if j not in set(p.pi[0, 0].tolist()))
    p.k[0, near, :64] = p.k[0, match, :64]
    p.k[0, near, 0] *= -1
    assert "gap" in (_refused(lambda: SP.conditions(p)) or "")
    p = fresh()
    i = int((p.pi[0, 0] == 76).nonzero()[0])                          # the query of the last x key now selects another x key
    other = next(j for j in range(1, 76) if j not in set(p.pi[0, 0].tolist()))
    p.q[0, i, :64] = p.b * p.k[0, other, :64] / p.a
    p.pi[0, 0, i] = other
    p.expect[0, i, :64] = p.v[0, other, :64].to(torch.float64)
    assert "forced keys" in (_refused(lambda: SP.conditions(p)) or "")
    SP._DRAWS.clear()


@pytest.mark.parametrize("run", SP.RUNS, ids=IDS)
def test_emulation_gives_the_expected_bits(run):
    p = SP.problem(*run)
    S.exact_rows(SP.emulate(p).to(BF16), p.expect, p.id, H=p.H, v=p.v)


def _mutants(p):
    t, n = p.t_x, p.n
    m = {"the latent keys' V rows read from the x segment": dict(v_segment=True),
         "the latent keys' K rows read from the x segment": dict(k_segment=True),
         "the last x key treated as padding": dict(drop=(t - 1,)),
         "the first latent key treated as padding": dict(drop=(t,)),
         "the last latent key treated as padding": dict(drop=(t + n - 1,)),
         "key 0 treated as padding": dict(drop=(0,)),
         "the latent V rows shifted by one": dict(shift_l=True)}
    if t % SP.KEY_TILE:
        m["the ragged tile's first key treated as padding"] = dict(drop=(t // SP.KEY_TILE * SP.KEY_TILE,))
    if p.H > 1:
        m["one head reads another head's V^T"] = dict(head_v=(0, 1))
    if p.B > 1:
        m["one sample reads another sample's keys"] = dict(sample_k=(1, 0))
    return m


@pytest.mark.parametrize("run", [r for r in SP.RUNS if r[:4] in ((2, 12, 16, 257), (2, 2, 5, 77), (2, 2, 3, 1))], ids=lambda r: SP.run_id(*r))
def test_exact_rows_refuses_the_mutants(run):
    """Each fault inside the emulation: the clean arithmetic passes, the mutant is refused."""
    p = SP.problem(*run)
    S.exact_rows(SP.emulate(p).to(BF16), p.expect, p.id, H=p.H, v=p.v)
    for name, mutant in _mutants(p).items():
        msg = _refused(lambda: S.exact_rows(SP.emulate(p, mutant).to(BF16), p.expect, name, H=p.H, v=p.v))
        assert msg is not None and ("differ from the selected row" in msg or "non-finite" in msg), f"{p.id}: {name}: not refused"
