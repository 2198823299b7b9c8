"""Every GroupNorm and LayerNorm kernel form on integer operands: the two moments each form publishes are the EXACT integers, and
every output is the bf16 of a float64 reference built from them (tests/_exact_norm.py).

tests/test_ops_gpu.py holds these kernels to atol 2e-2 on the output and 1e-3 on {mean, rstd}; a ragged part that loses its last
pixels, a chunk counted twice in the ordered finalize, a part normalised with stale statistics or a LayerNorm lane that misses its
last vector stays far below that (tests/test_norm_exact_cpu.py replays them), and the bit-reproducibility checks repeat the same
wrong sum.  Here x is drawn from non-zero small integers: S = sum x and Q = sum x^2 of a group are integers below 2^21 / 2^19 that
fp32 adds exactly in any order, for any part count, chunking or placement, and a dropped or doubled term moves Q by at least 1.

  test_group_norm_exact            every entry of test_ops_gpu.GROUP_NORM_CASES (no sync block, gn_impl as listed), every entry of
                                   GROUP_NORM_CLUSTER_CASES in both forms (the cluster form at gn_xmap 1 / 0, the row-major form at
                                   gn_rows_q default / 0 / 1 / 2) and MORE_CASES; each launch: the form it names ran (signs below),
                                   check_stats, check_partials, check_out, no workgroup gave up, guard bands intact
  test_recorded_group_norm_exact   every recorded signature (_layer_walk.family_cases("group_norm")) at batch 1, operands as
                                   Emitter.group_norm passes them, default options.  LARGE (cnt >= 2^19: the VAE's largest
                                   stages, where Q of even a +-1 draw leaves check_stats' reach) get the S half of check_stats,
                                   check_partials - the exact Q where the three-launch path runs, which is every one of them but
                                   65536x256 (eight parts of 8192 pixels: `partials` stays NaN) - and check_out, whose reference
                                   needs no bound on Q:
                                     gn 65536x512 silu, gn 65536x256 silu, gn 262144x256 silu, gn 262144x128 silu, gn 36864x512 silu,
                                     gn 147456x512 silu, gn 147456x256 silu, gn 589824x256 silu, gn 589824x128 silu
  test_layer_norm_exact            LN_CASES (every NV, its first partial vector, row counts that are no multiple of the four rows a
                                   workgroup takes) and the recorded text-encoder launch (77 x 768)
  test_one_wrong_pixel_is_seen     one case per GroupNorm form, ONE element of the uploaded x changed between magnitude 1 and 2: the
                                   checks raise and name the group; the recovered integers are off by exactly +-1 and +-3

Which form ran is read from three signs: the group tickets of the sync block (slot 3 g + log2 P - 1 of sample b holds P after one
cluster launch), the row-major ticket (256 after one launch) and the number of chunks written to `partials`; every case NAMES the
form it expects and _exact_norm.gn_form (the host rule of msd_group_norm restated) must give that name and those signs.

Forms against cases (G n: GROUP_NORM_CASES[n]; Cg n / Cr n: GROUP_NORM_CLUSTER_CASES[n] in the "groups" / "rows" form; M n: MORE_CASES[n]):
  gn_group_kernel<NPT, V>     <2,1> G0 M3 M9   <2,4> G2 G4 M4   <4,2> G1 G3   <8,4> G10   <16,1> G6 G8   <16,2> G7 G9
  gn_cluster_kernel<NPT, V>   <2,1> M7 M11   <2,2> Cg6   <2,4> Cg5 Cg7   <4,1> Cg0 M5   <4,2> Cg2   <4,4> Cg4 Cr4   <8,1> Cg1 Cr1 Cg3
                              <16,1> M14;  P = 2 Cg7 M11 M14, 4 Cg6 M7, 8 the rest;  XCD dealing on: Cg0-Cg4 Cg6 M5, off: Cg5 Cg7
                              (batch x P no power of two >= 8) M7 M11 M14 and every case again at gn_xmap = 0
  gn_rows_kernel<NPT>         <2> M12   <4> M2   <6> Cr0 Cr2 Cr3 Cr5 Cr6 Cr7 M6 M8;  P = 4 M2 M12, 8 Cr7 M8, 16 Cr6, 32 Cr0 M6, 64 Cr2
                              Cr3 Cr5;  Q = 1 / 2 / 4 each through gn_rows_q
  three launches, narrow      gn_stats<1, 256> + gn_apply<1, fused, 256>: G14 G15 M0 M10 M13; gn_stats<1, 256> + gn_finalize +
                              gn_apply<1, not fused, 256>: G5; gn_stats<2, 256> + gn_finalize + gn_apply<2, not fused, 256>: M15
  three launches, wide fused  gn_stats<1, 1024> on chunks four times coarser than gn_apply<1, fused, 1024>'s: G11 G12 G13 M1
  The non-fused wide branch of msd_group_norm (gn_finalize behind gn_stats<1, 1024>) cannot be reached: wide means hw C <= 4 Mi, hence a
  target of 128 chunks, hence at most 128 chunks, hence fused (gn_form asserts it).
  layer_norm_kernel<NV>       NV 1: 8, 320, 512   2: 520, 768, 1024   3: 1032, 1536   4: 1544, 2048
What MORE_CASES adds: odd channels per group (C = 96, 160: M0 M1 M2), a concat boundary at c0 = 8 inside group 0 (M3 M4 M7 M8 M10),
a prime hw (M5 M6 M11), hw = 7 below one pass of a workgroup (M9 M12 M13; gn_cluster admits no fewer than 64 pixels a part, so the
cluster form's smallest is M11: 131 pixels, a third of a pass per part), 16 units per thread in the cluster form (M14), two channel
vectors per thread through the separate finalize (M15)."""
import types

import pytest
import torch

import _exact_norm as N
import _extents as X
import _guard as G
import _layer_walk as LW
from conftest import run_calls
from test_ops_gpu import GROUP_NORM_CASES, GROUP_NORM_CLUSTER_CASES

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
NAN = float("nan")

# each at the smallest shape that reaches its form by the host rule; sync: a sync block is lent; the rest are set_option values
MORE_CASES = [
    dict(B=1, hw=100, c0=96, silu=True),                                  # 0  3 channels per group: three launches (no even unit)
    dict(B=1, hw=6557, c0=160, silu=False),                               # 1  5 channels per group on the wide fused form, ragged
    dict(B=1, hw=1031, c0=96, silu=True, sync=True, rows=1),              # 2  3 channels per group, row-major: vectors straddle groups
    dict(B=1, hw=64, c0=8, c1=312, silu=True),                            # 3  x0 is ONE 8-channel vector, the boundary inside group 0
    dict(B=1, hw=64, c0=8, c1=1272, silu=False),                          # 4  ... with 16-byte units: group 0's first unit is all of x0
    dict(B=1, hw=4099, c0=320, silu=True, sync=True, rows=0),             # 5  prime hw on 8 parts
    dict(B=1, hw=4099, c0=320, silu=True, sync=True, rows=1),             # 6  prime hw on 32 row-major parts
    dict(B=1, hw=1031, c0=8, c1=312, silu=True, sync=True, rows=0),       # 7  c0 = 8 on 4 parts, prime hw
    dict(B=1, hw=1031, c0=8, c1=312, silu=False, sync=True, rows=1),      # 8  c0 = 8 row-major: chunk 0 of every row is x0, the rest x1
    dict(B=2, hw=7, c0=320, silu=True),                                   # 9  fewer pixels than one pass of the workgroup
    dict(B=1, hw=1031, c0=8, c1=312, silu=True, impl=0),                  # 10 c0 = 8 on three launches
    dict(B=2, hw=131, c0=320, silu=True, sync=True, cluster=64, rows=0),  # 11 the fewest pixels gn_cluster admits: two parts of 66 / 65, a third of a pass
    dict(B=2, hw=7, c0=320, silu=False, sync=True, rows=1),               # 12 hw = 7 on four row-major parts of 2, 2, 2 and 1 pixels
    dict(B=2, hw=7, c0=320, silu=True, impl=0),                           # 13 hw = 7 as one chunk
    dict(B=1, hw=1201, c0=640, c1=320, silu=True, sync=True, cluster=600, rows=0),   # 14 two parts of 601 / 600 pixels: 9 passes of 68
    dict(B=1, hw=1101, c0=4096, silu=False),                              # 15 512 channel vectors: 2 per thread; 276 chunks, the last of 1 pixel
]

# the form each case names, at its own options (kept next to the lists: a list entry can never stop reaching its form unnoticed)
G_FORMS = ["group<2,1>", "group<4,2>", "group<2,4>", "group<4,2>", "group<2,4>", "three<1> finalize 1024 chunks", "group<16,1>", "group<16,2>",
           "group<16,1>", "group<16,2>", "group<8,4>", "three wide fused 32/128 chunks", "three wide fused 32/128 chunks",
           "three wide fused 32/125 chunks", "three<1> fused 64 chunks", "three<1> fused 3 chunks"]
CG_FORMS = ["cluster<4,1> P=8 xcd", "cluster<8,1> P=8 xcd", "cluster<4,2> P=8 xcd", "cluster<8,1> P=8 xcd", "cluster<4,4> P=8 xcd", "cluster<2,4> P=8",
            "cluster<2,2> P=4 xcd", "cluster<2,4> P=2"]
CR_FORMS = ["rows<6> P=32 Q=4", "cluster<8,1> P=8 xcd", "rows<6> P=64 Q=4", "rows<6> P=64 Q=2", "cluster<4,4> P=8 xcd", "rows<6> P=64 Q=2",
            "rows<6> P=16 Q=4", "rows<6> P=8 Q=4"]
M_FORMS = ["three<1> fused 2 chunks", "three wide fused 32/127 chunks", "rows<4> P=4 Q=4", "group<2,1>", "group<2,4>", "cluster<4,1> P=8 xcd",
           "rows<6> P=32 Q=4", "cluster<2,1> P=4", "rows<6> P=8 Q=4", "group<2,1>", "three<1> fused 43 chunks", "cluster<2,1> P=2",
           "rows<2> P=4 Q=4", "three<1> fused 1 chunks", "cluster<16,1> P=2", "three<2> finalize 276 chunks"]


def _case(tag, c, form, **kw):
    d = dict(B=c["B"], hw=c["hw"], c0=c["c0"], c1=c.get("c1", 0), silu=c["silu"], sync=c.get("sync", False), form=form, id=tag,
             opt={k: c[k] for k in ("impl", "cluster", "rows") if k in c})
    d.update(kw)
    return d


EXACT_CASES = ([_case(f"G{i}", c, G_FORMS[i]) for i, c in enumerate(GROUP_NORM_CASES)]
               + [_case(f"Cg{i}", c, CG_FORMS[i], sync=True, opt=dict(cluster=c.get("opt", 256), rows=0)) for i, c in enumerate(GROUP_NORM_CLUSTER_CASES)]
               + [_case(f"Cr{i}", c, CR_FORMS[i], sync=True, opt=dict(cluster=c.get("opt", 256), rows=1)) for i, c in enumerate(GROUP_NORM_CLUSTER_CASES)]
               + [_case(f"M{i}", c, M_FORMS[i]) for i, c in enumerate(MORE_CASES)])
LN_CASES = [(5, 8), (7, 320), (4, 512), (9, 520), (6, 1024), (3, 1032), (5, 1536), (6, 1544), (7, 2048)]
RECORDED = list(LW.family_cases("group_norm"))
RECORDED_LN = list(LW.family_cases("layer_norm"))
# one case per form for test_one_wrong_pixel_is_seen
WRONG_PIXEL_CASES = ["G0", "Cg6", "Cr7", "G14", "M1", "M15"]


def problem_id(c):
    """The draw depends on the operands alone: the same tensor for a shape in whatever form it runs."""
    return "gn/%dx%dx%d|%d%s" % (c["B"], c["hw"], c["c0"], c["c1"], "/silu" if c["silu"] else "")


def case_problem(c):
    return N.gn_problem(c["B"], c["hw"], c["c0"], c["c1"], c["silu"], problem_id(c))


def variants(c):
    """The option sets a case is launched at: the cluster form with and without the XCD dealing, the row-major form at every channel
    share (placement only: the same exact moments and the same outputs are asked of each)."""
    kind = N.gn_form(c["B"], c["hw"], c["c0"] + c["c1"], c["sync"], **c["opt"]).kind
    if c["id"][0] != "C":
        return [{}]
    return [{}, dict(xmap=0)] if kind == "cluster" else [{}, dict(rows_q=0), dict(rows_q=1), dict(rows_q=2)]


def recorded_problem(s):
    sid = LW.family_id("group_norm", s)
    return N.gn_problem(1, s.hw, s.c0, s.c1, s.silu, "recorded/" + sid, large=s.hw * ((s.c0 + s.c1) // 32) >= N.Q_MAX)


def set_options(lib, opt):
    o = dict(N.GN_DEFAULTS, **opt)
    for k, v in o.items():
        assert lib.msd_set_option(("gn_" + k).encode(), v) == 0, (k, v)


def launch(gpu, p, sync, x=None):
    """One guarded msd_group_norm launch on problem p (x: the tensor to upload instead of p.x): (guard, out, stats, partials, sync)."""
    from minsdtf_amd import ops

    geo = dict(batch=p.B, hw=p.hw, c0=p.c0, c1=p.c1)
    g = G.Guard(gpu, X.group_norm(x0=1, x1=1 if p.c1 else None, gamma=1, beta=1, stats=1, partials=1, out=1, sync=1 if sync else None, **geo))
    xd = (p.x if x is None else x).to(gpu)
    x0 = g.out((p.B, p.hw, p.c0), BF16, 0.0, "x0")
    x0.copy_(xd[..., :p.c0])
    x1 = None
    if p.c1:
        x1 = g.out((p.B, p.hw, p.c1), BF16, 0.0, "x1")
        x1.copy_(xd[..., p.c0:])
    del xd
    out = g.out((p.B, p.hw, p.C), BF16, NAN, "out")
    stats = g.out((p.B, 32, 2), torch.float32, NAN, "stats")
    partials = g.out((p.B * ops.GN_MAX_CHUNKS, 64), torch.float32, NAN, "partials")
    sy = g.out((p.B * ops.GN_SYNC_WORDS_PER_SAMPLE // 64, 64), torch.int32, 0, "sync") if sync else None
    run_calls(ops.group_norm(x0=x0, x1=x1, gamma=g.inp(p.gamma, "gamma"), beta=g.inp(p.beta, "beta"), stats=stats, partials=partials, out=out,
                             silu=p.silu, eps=N.EPS, sync=sy, **geo))
    return g, out, stats, partials, sy


def assert_form(form, B, partials, sync, S, Q, what):
    """The signs the launch left are those of `form`; check_partials on the way.  No workgroup gave up."""
    nchunks = N.check_partials(partials, B, S, Q, what, written=form.kind == "three")
    assert nchunks == form.nchunks, f"{what}: {nchunks} chunks in `partials`, {form.name} writes {form.nchunks}"
    if sync is None:
        assert form.kind in ("group", "three"), what
        return
    words = sync.view(B, -1, 64)
    assert int(words[:, :97, 8].max()) == 0, f"{what}: a workgroup gave up waiting for its partial moments"
    tickets = words[:, :96, 0].reshape(B, 32, 3).cpu()
    want = torch.zeros(B, 32, 3, dtype=torch.int32)
    if form.kind == "cluster":
        want[:, :, form.parts.bit_length() - 2] = form.parts
    assert torch.equal(tickets, want), f"{what}: group tickets {tickets[0, 0].tolist()} (sample 0, group 0; P = 2, 4, 8), {form.name} expected"
    rows_ticket = sync.view(B, -1)[:, 96 * 64].cpu()
    assert rows_ticket.tolist() == [256 if form.kind == "rows" else 0] * B, f"{what}: row-major ticket {rows_ticket.tolist()}, {form.name} expected"


def report(what, form, q_err, ties, out_err):
    print(f"\nRECORD | {form} | {what} | q_err {q_err:.2f} x 2^-24 | other neighbour {ties[0]}/{ties[1]} near ties | out_err {out_err:.4f} bf16 ulp")


@pytest.mark.parametrize("c", EXACT_CASES, ids=[c["id"] for c in EXACT_CASES])
def test_group_norm_exact(gpu, c):
    from minsdtf_amd import _lib

    lib = _lib.load()
    p = case_problem(c)
    try:
        for v in variants(c):
            opt = dict(c["opt"], **v)
            form = N.gn_form(p.B, p.hw, p.C, c["sync"], **opt)
            if not v:
                assert form.name == c["form"], f"{c['id']}: names {c['form']}, the host rule gives {form.name}"
            what = f"{c['id']} {problem_id(c)} {opt} [{form.name}]"
            set_options(lib, opt)
            g, out, stats, partials, sync = launch(gpu, p, c["sync"])
            assert_form(form, p.B, partials, sync, p.S, p.Q, what)
            q_err = N.check_stats(stats, p.S, p.Q, p.cnt, what)
            ties, out_err = N.check_out(out, p.x, (p.y, p.tol), what)
            g.check()
            report(what, form.name, q_err, ties, out_err)
            del g, out, stats, partials, sync
    finally:
        set_options(lib, {})


@pytest.mark.parametrize("s", RECORDED, ids=[LW.family_id("group_norm", s) for s in RECORDED])
def test_recorded_group_norm_exact(gpu, s):
    p = recorded_problem(s)
    form = N.gn_form(1, s.hw, p.C, s.sync)
    what = f"{LW.family_id('group_norm', s)} [{form.name}]"
    g, out, stats, partials, sync = launch(gpu, p, s.sync)
    assert_form(form, 1, partials, sync, p.S, p.Q, what)
    q_err = N.check_stats(stats, p.S, p.Q, p.cnt, what, q_half=not p.large)
    ties, out_err = N.check_out(out, p.x, (p.y, p.tol), what)      # (on the device: the largest output is 151 M values)
    g.check()
    report(what, form.name, q_err, ties, out_err)
    del g, out, stats, partials, sync
    torch.cuda.empty_cache()


@pytest.mark.parametrize("rows,c", LN_CASES + [(s.rows_per_sample, s.c) for s in RECORDED_LN])
def test_layer_norm_exact(gpu, rows, c):
    from minsdtf_amd import ops

    p = N.ln_problem(rows, c, f"ln/{rows}x{c}")
    g = G.Guard(gpu, X.layer_norm(x=1, gamma=1, beta=1, out=1, rows=rows, c=c))
    out = g.out((rows, c), BF16, NAN, "out")
    run_calls(ops.layer_norm(x=g.inp(p.x.to(BF16), "x"), gamma=g.inp(p.gamma, "gamma"), beta=g.inp(p.beta, "beta"), out=out, rows=rows, c=c, eps=N.EPS))
    ties, out_err = N.check_ln_out(out, p, f"ln {rows}x{c}")
    g.check()
    report(f"ln {rows}x{c}", f"layer_norm<{(c // 8 + 63) // 64}>", 0.0, ties, out_err)


@pytest.mark.parametrize("where", ["last pixel", "first pixel of the last part"])
@pytest.mark.parametrize("cid", WRONG_PIXEL_CASES)
def test_one_wrong_pixel_is_seen(gpu, cid, where):
    """The checks end to end, on the device: the launch runs on valid operands that differ from the reference's x in ONE element (the
    last channel of the last group, of the last sample; its magnitude changed between 1 and 2: S moves by +-1, Q by +-3).  The
    statistics and `partials` are exact for what was uploaded; against the reference they are refused, the message names the group,
    and the recovered integers are off by exactly those deltas in that group alone.  check_out sees the one pixel."""
    from minsdtf_amd import _lib

    lib = _lib.load()
    c = next(k for k in EXACT_CASES if k["id"] == cid)
    p = case_problem(c)
    form = N.gn_form(p.B, p.hw, p.C, c["sync"], **c["opt"])
    assert form.name == c["form"]
    px = p.hw - 1 if where == "last pixel" else (-(-p.hw // form.ppart) - 1) * form.ppart
    assert 0 <= px < p.hw and (where == "last pixel" or px + form.ppart >= p.hw)
    b, ch = p.B - 1, p.C - 1
    x = p.x.clone()
    old = int(x[b, px, ch])
    new = (3 - abs(old)) * (1 if old > 0 else -1)
    x[b, px, ch] = new
    dS, dQ = new - old, new * new - old * old
    assert abs(dS) == 1 and abs(dQ) == 3
    S2, Q2 = N.gn_moments(x)
    try:
        set_options(lib, c["opt"])
        g, out, stats, partials, sync = launch(gpu, p, c["sync"], x=x)
    finally:
        set_options(lib, {})
    what = f"{cid} [{form.name}], one pixel changed"
    assert_form(form, p.B, partials, sync, S2, Q2, what)
    N.check_stats(stats, S2, Q2, p.cnt, what)
    g.check()
    with pytest.raises(AssertionError, match=rf"sample {b}, group 31: "):
        N.check_stats(stats, p.S, p.Q, p.cnt, what)
    S_rec, Q_rec = N.recover(stats, p.cnt)
    want_S, want_Q = torch.zeros(p.B, 32, dtype=torch.int64), torch.zeros(p.B, 32, dtype=torch.int64)
    want_S[b, 31], want_Q[b, 31] = dS, dQ
    assert torch.equal(S_rec.round().to(torch.int64) - p.S, want_S) and torch.equal(Q_rec.round().to(torch.int64) - p.Q, want_Q)
    if form.kind == "three":
        with pytest.raises(AssertionError, match=rf"sample {b}, group 31: "):
            N.check_partials(partials, p.B, p.S, p.Q, what)
    with pytest.raises(AssertionError, match=rf"sample {b}, channel {ch} \(group 31\)"):
        N.check_out(out, p.x, (p.y, p.tol), what)
    N.check_out(out, x, (N.gn_ref_terms(_with_moments(p, S2, Q2))), what, values=(-2, -1, 1, 2))


def _with_moments(p, S, Q):
    """p's reference terms from other exact moments (the uploaded tensor's), on all four values."""
    q = types.SimpleNamespace(**vars(p))
    q.values = (-2, -1, 1, 2)
    q.mean, q.var, q.rstd, q.a, q.shift = N.gn_reference(S, Q, p.cnt, p.gamma, p.beta)
    return q
