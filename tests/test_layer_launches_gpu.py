"""Every msd_group_norm, msd_attention, msd_cross_attention_q, msd_conv_direct and msd_layer_norm launch a default job records, at
its real shape, next to its own high-precision answer.

tests/test_layer_shapes_gpu.py does this for msd_conv_gemm, where the ENGINE picks the kernel form.  For the families here the
LIBRARY picks it, from the launch's real size and its default options: five GroupNorm forms by hw, C, the batch and the sync block;
64, 128 or 256 queries per attention workgroup and the partial-round split by the grid size and the device's CU count.
tests/test_ops_gpu.py forces those choices at sizes of its own; this module sets no option at all and launches what the
tensor-less walk of the emitters records (tests/_layer_walk.py: one case per signature, at every batch it was walked at), operands
as the emitters pass them, each between guard bands (tests/_guard.py) sized by the header's extents (tests/_extents.py).  Draws,
references and bounds live in tests/_layer_draw.py, where tests/test_layer_cases_cpu.py shows that they refuse a wrong result.  A
failure names the launch, not the image."""
import gc

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _extents as X
import _guard as G
import _layer_draw as D
import _layer_walk as LW
from conftest import run_calls
from test_layer_shapes_gpu import _row_moments
from test_ops_gpu import bf, close, conv_ref

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
NAN = float("nan")
NORMS, ATTNS, XATTNS, DIRECTS, LNS = (LW.family_cases(f) for f in ("group_norm", "attention", "cross_attention_q", "conv_direct", "layer_norm"))
_ran = {f: set() for f in LW.EXPECTED_FAMILY_CASES}


def _ids(family, cases):
    return [LW.family_id(family, s) for s in cases]


def _done(family, sid):
    _ran[family].add(sid)
    gc.collect()
    torch.cuda.empty_cache()


def _same_samples(got, first, b, Bmax, what):
    """One numerics class per launch: sample i of the batch-b launch carries the bits it has in the largest batch (compared on the
    device, every sample - samples 0 and b - 1 among them)."""
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[got.element_size()]
    for i in range(b):
        assert torch.equal(got[i].view(view), first[i].view(view)), f"{what}: sample {i} of batch {b} differs from its bits at batch {Bmax}"


@pytest.mark.parametrize("sig", list(NORMS), ids=_ids("group_norm", NORMS))
def test_group_norm_launch(gpu, sig):
    """One recorded GroupNorm at every batch it was walked at, operands as Emitter.group_norm passes them (a zeroed sync block of
    batch * GN_SYNC_WORDS_PER_SAMPLE words, partials of batch * GN_MAX_CHUNKS * 64 floats, stats of batch * 64 floats, x1 where the
    input is a concat): output and {mean, rstd} within test_group_norm's bounds of the float64-statistics reference; a second
    launch on the same sync block (the next epoch) gives the same bits; no workgroup gave up waiting; a sample's bits do not depend
    on its batch (norm.hip: "a sample's result must not depend on the batch it is computed in")."""
    from minsdtf_amd import ops

    s, sid, dev = sig, LW.family_id("group_norm", sig), gpu
    per = NORMS[s]
    Bmax = max(per)
    C = s.c0 + s.c1
    gamma, beta = D.gn_affine(s, sid)
    gw = G.Guard(dev, X.group_norm(gamma=1, beta=1, batch=1, hw=s.hw, c0=s.c0, c1=s.c1))
    gd, bd = gw.inp(gamma, "gamma"), gw.inp(beta, "beta")
    xs = [D.gn_draw_sample(s, sid, i) for i in range(Bmax)]
    first = first_stats = None
    for b in sorted(per, reverse=True):
        assert len(per[b]) == 1
        geo = dict(batch=b, hw=s.hw, c0=s.c0, c1=s.c1)
        g = G.Guard(dev, X.group_norm(x0=1, x1=1 if s.c1 else None, stats=1, partials=1, out=1, sync=1 if s.sync else None, **geo))
        x0 = g.out((b, s.hw, s.c0), BF16, 0.0, "x0")
        x1 = g.out((b, s.hw, s.c1), BF16, 0.0, "x1") if s.c1 else None
        for i in range(b):
            x0[i].copy_(xs[i][:, :s.c0])
            if s.c1:
                x1[i].copy_(xs[i][:, s.c0:])
        stats = g.out((b, 32, 2), torch.float32, NAN, "stats")
        partials = g.out((b * ops.GN_MAX_CHUNKS, 64), torch.float32, NAN, "partials")
        sync = g.out((b * ops.GN_SYNC_WORDS_PER_SAMPLE // 64, 64), torch.int32, 0, "sync") if s.sync else None
        out = g.out((b, s.hw, C), BF16, NAN, "out")
        out2 = g.out((b, s.hw, C), BF16, NAN, "out", label="out again")
        kw = dict(x0=x0, x1=x1, gamma=gd, beta=bd, stats=stats, partials=partials, silu=s.silu, eps=D.EPS, sync=sync, **geo)
        run_calls(ops.group_norm(out=out, **kw))
        st = stats.clone()
        stats.fill_(NAN)
        run_calls(ops.group_norm(out=out2, **kw))
        what = f"{sid} | batch {b}"
        assert torch.equal(out.view(torch.int16), out2.view(torch.int16)), f"{what}: the next epoch on the same sync block gives other bits"
        assert torch.equal(stats.view(torch.int32), st.view(torch.int32)), f"{what}: the next epoch gives other statistics"
        if sync is not None:   # (word 8 of the 96 group slots and of the row-major form's header slot of every sample)
            assert int(sync.view(b, -1, 64)[:, :97, 8].max()) == 0, f"{what}: a workgroup gave up waiting for its partial moments"
        if first is None:
            first, first_stats = out, st
            got, gst = out.cpu(), st.cpu()
            for i in range(b):   # the reference, sample by sample (the largest is 151 M values)
                ref, mean, rstd = D.gn_reference(s, xs[i], gamma, beta)
                D.gn_compare(got[i], gst[i], ref, mean, rstd, f"{what} sample {i}")
                del ref
            del got
        else:
            _same_samples(out, first, b, Bmax, what)
            _same_samples(st, first_stats, b, Bmax, what + " statistics")
        g.check()
        del g, x0, x1, out2, partials, sync, kw, stats
        if out is not first:
            del out
    gw.check()
    del first, xs
    _done("group_norm", sid)


@pytest.mark.parametrize("sig", list(ATTNS), ids=_ids("attention", ATTNS))
def test_attention_launch(gpu, sig):
    """One recorded msd_attention at every batch it was walked at, operands as the engine records them (q_ld = k_ld = o_ld = C, vt_ld
    as walked with NaN in V^T's padding columns, q prescaled where the record says so, for d = 512 a workspace of exactly the
    recorded floats): the fp32 softmax on the bf16-rounded inputs within test_attention's bounds - every query of (sample 0, head
    0) and (last sample, last head), the first 256, the last 256 and every 37th query of every other pair - and a sample's bits do
    not depend on its batch (attention.hip, msd_attention: the workgroup size is "scheduling only")."""
    from minsdtf_amd import ops

    s, sid, dev = sig, LW.family_id("attention", sig), gpu
    per = ATTNS[s]
    Bmax = max(per)
    H, d, S, T = s.heads, s.head_dim, s.s, s.t
    C = H * d
    draws = [D.attn_draw_sample(s, sid, i) for i in range(Bmax)]
    first = None
    for b in sorted(per, reverse=True):
        assert len(per[b]) == 1
        l = per[b][0]
        geo = dict(batch=b, heads=H, head_dim=d, s=S, t=T, q_ld=s.q_ld, k_ld=s.k_ld, vt_ld=s.vt_ld, o_ld=s.o_ld)
        g = G.Guard(dev, X.attention(q=1, k=1, vt=1, out=1, workspace=1 if l.workspace_floats else None, **geo))
        q = g.out((b * S, C), BF16, 0.0, "q")
        k = g.out((b * T, C), BF16, 0.0, "k")
        vt = g.out((b, C, s.vt_ld), BF16, 0.0, "vt")
        for i in range(b):
            q[i * S:(i + 1) * S].copy_(draws[i][0])
            k[i * T:(i + 1) * T].copy_(draws[i][1])
            vt[i, :, :T].copy_(draws[i][2].t())
        for name in ("q", "k", "vt"):
            next(o for o in g.operands if o.label == name).role = "in"
        g.gaps(vt, T)                # V^T's padding keys hold NaN: what the arena's previous tenant may have left
        out = g.out((b, S, C), BF16, NAN, "out")
        kw = dict(q=q, k=k, vt=vt, out=out, scale=s.scale, causal=s.causal, q_prescaled=s.q_prescaled, **geo)
        if l.workspace_floats:
            assert l.workspace_floats == X.attention_workspace_floats(b, H, S)
            kw.update(workspace=g.out((l.workspace_floats // (d + 2), d + 2), torch.float32, NAN, "workspace"), workspace_floats=l.workspace_floats)
        run_calls(ops.attention(**kw))
        what = f"{sid} | batch {b}"
        if first is None:
            first = out
            got = out.cpu()
            for (i, h, idx) in D.attn_blocks(b, H, S):
                ref = D.attn_reference(s, *draws[i], h, idx)
                D.attn_compare(got[i, idx, h * d:(h + 1) * d], ref, f"{what} sample {i} head {h} ({idx.numel()} queries)")
            del got
        else:
            assert bool(torch.isfinite(out.float()).all()), f"{what}: non-finite outputs"
            _same_samples(out, first, b, Bmax, what)
        g.check()
        del g, q, k, vt, kw
        if out is not first:
            del out
    del first, draws
    _done("attention", sid)


@pytest.mark.parametrize("sig", list(XATTNS), ids=_ids("cross_attention_q", XATTNS))
def test_cross_attention_q_launch(gpu, sig):
    """One recorded msd_cross_attention_q at every batch it was walked at: ln_in partials as the producing GEMM leaves them, with the
    walked slot count, folded to_q weights in the walked layout, against LayerNorm -> Dense -> softmax(q k^T) v in fp32 within
    test_cross_attention_q's bound; a sample's bits do not depend on its batch."""
    from minsdtf_amd import ops, packing

    s, sid, dev = sig, LW.family_id("cross_attention_q", sig), gpu
    per = XATTNS[s]
    Bmax = max(per)
    H, d, S, T = s.heads, s.head_dim, s.s, s.t
    C = H * d
    gamma, beta, wq = D.xattn_weights(s, sid)
    wf, cs, cb = packing.fold_layer_norm(wq.t().contiguous(), None, gamma.numpy(), beta.numpy(), dev)
    gw = G.Guard(dev, X.cross_attention_q(wq=1, ln_colsum=1, bias=1, batch=1, heads=H, head_dim=d, s=S, t=T, k_ld=s.k_ld, vt_ld=s.vt_ld, o_ld=s.o_ld, ln_in_slots=1))
    layouts = {}
    cs, cb = gw.inp(cs, "ln_colsum"), gw.inp(cb, "bias")
    draws = [D.xattn_draw_sample(s, sid, i) for i in range(Bmax)]
    first = None
    for b in sorted(per, reverse=True):
        for l in per[b]:
            geo = dict(batch=b, heads=H, head_dim=d, s=S, t=T, k_ld=s.k_ld, vt_ld=s.vt_ld, o_ld=s.o_ld, ln_in_slots=l.ln_in_slots)
            g = G.Guard(dev, X.cross_attention_q(x=1, ln_in=1, k=1, vt=1, out=1, **geo))
            if l.w_layout not in layouts:
                layouts[l.w_layout] = gw.inp(packing.chunk_major(wf) if l.w_layout else wf, "wq", label=f"wq layout {l.w_layout}")
            x = g.inp(torch.cat([draws[i][0] for i in range(b)]).to(BF16), "x")
            stats = g.inp(torch.cat([_row_moments(draws[i][0], l.ln_in_slots) for i in range(b)]), "ln_in")
            k = g.inp(torch.cat([draws[i][1] for i in range(b)]).to(BF16), "k")
            vtf = torch.zeros(b, C, s.vt_ld, dtype=BF16)
            for i in range(b):
                vtf[i, :, :T] = draws[i][2].t().to(BF16)
            vt = g.inp(vtf, "vt")
            g.gaps(vt, T)
            out = g.out((b, S, C), BF16, NAN, "out")
            run_calls(ops.cross_attention_q(x=x, ln_in=stats, wq=layouts[l.w_layout], ln_colsum=cs, bias=cb, k=k, vt=vt, out=out, ln_eps=D.EPS,
                                            w_layout=l.w_layout, **geo))
            what = f"{sid} | batch {b} slots {l.ln_in_slots} layout {l.w_layout}"
            if first is None:
                first = out
                got = out.cpu()
                for i in range(b):
                    D.xattn_compare(got[i], D.xattn_reference(s, *draws[i], gamma, beta, wq), f"{what} sample {i}")
                del got
            else:
                assert bool(torch.isfinite(out.float()).all()), f"{what}: non-finite outputs"
                _same_samples(out, first, b, Bmax, what)
            g.check()
            del g, x, stats, k, vt
            if out is not first:
                del out
    gw.check()
    del first, draws
    _done("cross_attention_q", sid)


@pytest.mark.parametrize("sig", list(DIRECTS), ids=_ids("conv_direct", DIRECTS))
def test_conv_direct_launch(gpu, sig):
    """One recorded msd_conv_direct at every batch it was walked at, against F.conv2d in fp32 with test_conv_direct's bounds (fp32
    output: rtol 1e-4, atol 1e-4 max|ref|; uint8 output: the truncating conversion, off by one at most and equal on > 99.5 %); a
    sample's bits do not depend on its batch."""
    from minsdtf_amd import ops

    s, sid, dev = sig, LW.family_id("conv_direct", sig), gpu
    per = DIRECTS[s]
    Bmax = max(per)
    in_f32 = s.in_dtype == ops.OUT_F32
    pad = 1 if s.ksize == 3 else 0
    gen = D.gen(sid, "weights")
    w = torch.randn(s.ksize, s.ksize, s.c_in, s.c_out, generator=gen) / (s.ksize * s.ksize * s.c_in) ** 0.5
    bias = torch.randn(s.c_out, generator=gen) * 0.1
    xs, rs, refs = [], [], []
    for i in range(Bmax):
        gi = D.gen(sid, "sample", i)
        x = torch.randn(s.h_in, s.w_in, s.c_in, generator=gi)
        xs.append(x if in_f32 else bf(x))
        ref = conv_ref(xs[i][None] * s.in_scale, w, bias, stride=s.stride, pad=pad)[0]
        if s.residual:
            rs.append(bf(torch.randn(*ref.shape, generator=gi)))
            ref = ref + rs[i]
        refs.append(ref)
    Ho, Wo = refs[0].shape[:2]
    dt = {ops.OUT_BF16: BF16, ops.OUT_F32: torch.float32, ops.OUT_U8: torch.uint8}[s.out_dtype]
    gw = G.Guard(dev, X.conv_direct(w=1, bias=1, batch=1, h_in=s.h_in, w_in=s.w_in, c_in=s.c_in, c_out=s.c_out, ksize=s.ksize, stride=s.stride))
    wd, bd = gw.inp(w, "w"), gw.inp(bias, "bias")
    first = None
    for b in sorted(per, reverse=True):
        assert len(per[b]) == 1 and per[b][0].in_batch_mod == b
        geo = dict(batch=b, in_batch_mod=b, h_in=s.h_in, w_in=s.w_in, c_in=s.c_in, c_out=s.c_out, ksize=s.ksize, stride=s.stride,
                   in_dtype=s.in_dtype, out_dtype=s.out_dtype)
        g = G.Guard(dev, X.conv_direct(x=1, residual=1 if s.residual else None, out=1, **geo))
        x = g.inp(torch.stack(xs[:b]).to(torch.float32 if in_f32 else BF16), "x")
        res = g.inp(torch.stack(rs[:b]).to(BF16), "residual") if s.residual else None
        out = g.out((b, Ho, Wo, s.c_out), dt, 0, "out")
        run_calls(ops.conv_direct(x=x, w=wd, bias=bd, residual=res, out=out, act=s.act, act_in=s.act_in, in_scale=s.in_scale, **geo))
        what = f"{sid} | batch {b}"
        if first is None:
            first = out
            got = out.cpu()
            for i in range(b):
                if s.out_dtype == ops.OUT_U8:
                    refu = np.clip(((refs[i].numpy() + 1.0) * 0.5) * 255.0, 0, 255)
                    gi = got[i].numpy().astype(np.int32)
                    # truncation: allow off-by-one where the fp32 value sits on an integer boundary
                    assert np.all(np.abs(gi - np.floor(refu)) <= 1), f"{what} sample {i}: uint8 conversion"
                    assert np.mean(gi == np.floor(refu).astype(np.int32)) > 0.995, f"{what} sample {i}: uint8 conversion"
                elif s.out_dtype == ops.OUT_F32:
                    close(got[i], refs[i], rtol=1e-4, atol=1e-4 * float(refs[i].abs().max()), what=f"{what} sample {i}")
                else:
                    close(got[i], refs[i], what=f"{what} sample {i}")
            del got
        else:
            _same_samples(out, first, b, Bmax, what)
        g.check()
        del g, x, res
        if out is not first:
            del out
    gw.check()
    del first, xs, rs, refs
    _done("conv_direct", sid)


@pytest.mark.parametrize("sig", list(LNS), ids=_ids("layer_norm", LNS))
def test_layer_norm_launch(gpu, sig):
    """The text encoder's msd_layer_norm (77 rows of 768 per prompt) at one and two prompts, as test_layer_norm draws and bounds it;
    a prompt's bits do not depend on its batch."""
    from minsdtf_amd import ops

    s, sid, dev = sig, LW.family_id("layer_norm", sig), gpu
    per = LNS[s]
    Bmax = max(per)
    R, c = s.rows_per_sample, s.c
    gen = D.gen(sid, "weights")
    gamma, beta = torch.randn(c, generator=gen) * 0.2 + 1, torch.randn(c, generator=gen) * 0.2
    xs = [bf(torch.randn(R, c, generator=D.gen(sid, "sample", i)) * 3 + 1) for i in range(Bmax)]
    gw = G.Guard(dev, X.layer_norm(gamma=1, beta=1, rows=R, c=c))
    gd, bd = gw.inp(gamma, "gamma"), gw.inp(beta, "beta")
    first = None
    for b in sorted(per, reverse=True):
        assert len(per[b]) == 1 and per[b][0].rows == b * R
        g = G.Guard(dev, X.layer_norm(x=1, out=1, rows=b * R, c=c))
        x = g.inp(torch.cat(xs[:b]).to(BF16), "x")
        out = g.out((b, R, c), BF16, NAN, "out")
        run_calls(ops.layer_norm(x=x, gamma=gd, beta=bd, out=out, rows=b * R, c=c, eps=D.EPS))
        what = f"{sid} | batch {b}"
        if first is None:
            first = out
            close(out, F.layer_norm(torch.stack(xs[:b]), (c,), gamma, beta, eps=D.EPS), atol=2e-2, what=what)
        else:
            _same_samples(out, first, b, Bmax, what)
        g.check()
    gw.check()
    _done("layer_norm", sid)


def test_every_counted_case_ran(gpu):
    """No recorded signature is left out, skipped or deselected: the walk's counts (kept by tests/test_layer_cases_cpu.py) are the
    numbers of cases that ran to their end in this session."""
    for f, cases in (("group_norm", NORMS), ("attention", ATTNS), ("cross_attention_q", XATTNS), ("conv_direct", DIRECTS), ("layer_norm", LNS)):
        assert len(cases) == LW.EXPECTED_FAMILY_CASES[f], f
        assert len(_ran[f]) == LW.EXPECTED_FAMILY_CASES[f], (f, sorted(set(_ids(f, cases)) - _ran[f]))
