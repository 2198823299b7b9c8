"""Every msd_conv_gemm launch the engines record, at its real shape, next to its own fp32 answer.

tests/test_ops_gpu.py checks the kernel families at toy sizes; whole-network PSNR checks the product.  This module checks ONE
production launch at a time: the case list is the tensor-less walk of the emitters (tests/_layer_walk.py: UNet, ControlNet, VAE
decoder and encoder at the tuned sizes and batches, plus untuned batches and an untuned size), one case per layer signature
(shape without its batch + epilogue).  A case launches exactly what the engine recorded at every batch the signature was
walked at - its kernel form, split-K, weight layout, a workspace of exactly splitk * M * N floats - and compares with the plain
PyTorch operation on the CPU, computed once at the largest batch.  A failure names the layer, not the image."""
import gc
import hashlib
import math

import pytest
import torch
import torch.nn.functional as F

import _extents as X
import _guard as G
import _layer_walk as LW
from conftest import run_calls
from test_ops_gpu import bf, close, conv_ref

pytestmark = pytest.mark.gpu

CASES = LW.cases()
IDS = [LW.sig_id(s) for s in CASES]
MEAN = 0.3     # mean of every drawn activation (std 1)
STEPS, STEP = 3, 2   # rows of the per-step row-vector table, the row the device step counter selects
_ran = set()


def _gen(sid, *what):
    g = torch.Generator()
    g.manual_seed(int.from_bytes(hashlib.sha256(repr((sid,) + what).encode()).digest()[:7], "little"))
    return g


def _act(g, *shape):
    return bf(torch.randn(*shape, generator=g) + MEAN)


def _draw(s, sid, B):
    """The operands of signature `s` for B samples; sample i is drawn from a generator seeded by (signature, i) alone, so it
    is the same tensor at every batch.  Weights and bias are seeded by the signature."""
    ho, wo = LW.out_hw(s)
    n_out = s.N // 2 if _geglu(s) else s.N
    per = []
    for i in range(B):
        g = _gen(sid, "sample", i)
        d = dict(a0=_act(g, s.h_in, s.w_in, s.c0))
        d["a1"] = _act(g, s.h_in, s.w_in, s.c1) if s.c1 else None
        d["a2"] = _act(g, ho, wo, s.c2) if s.c2 else None
        d["a3"] = _act(g, ho, wo, s.c3) if s.c3 else None
        d["res"] = bf(torch.randn(ho, wo, n_out, generator=g)) if s.residual else None
        d["rv"] = torch.randn(STEPS, s.N, generator=g) if s.rowvec else None
        per.append(d)
    t = {k: (torch.stack([p[k] for p in per]) if per[0][k] is not None else None) for k in per[0]}
    if t["rv"] is not None:
        t["rv"] = t["rv"].permute(1, 0, 2).contiguous()   # [STEPS][B][N]
    return t


def _geglu(s):
    from minsdtf_amd import ops

    return s.act == ops.ACT_GEGLU


def _weights(s, sid):
    """fp32 (bf16-rounded) weights: the main filter (kh, kw, cin, N) / sqrt(K), the shortcut's 1x1 / sqrt(cx), fp32 bias, and
    for a LayerNorm-fold consumer gamma / beta."""
    g = _gen(sid, "weights")
    cin, cx = s.c0 + s.c1, s.c2 + s.c3
    w = bf(torch.randn(s.ksize, s.ksize, cin, s.N, generator=g) / math.sqrt(s.ksize * s.ksize * cin))
    wsc = bf(torch.randn(1, 1, cx, s.N, generator=g) / math.sqrt(cx)) if cx else None
    bias = torch.randn(s.N, generator=g) * (0.1 if (s.ln_in or s.split or _geglu(s)) else 1.0)
    gamma, beta = 1 + 0.3 * torch.randn(cin, generator=g), 0.2 * torch.randn(cin, generator=g)
    return w, wsc, bias, gamma, beta


def _reference(s, t, w, wsc, bias, gamma, beta):
    """The plain operation on the CPU: fp32 for a bf16 output, float64 for an fp32 output.  Returns the output [B, ho, wo, N']."""
    from minsdtf_amd import ops

    dt = torch.float64 if s.out_dtype == ops.OUT_F32 else torch.float32
    x = (torch.cat([t["a0"], t["a1"]], dim=-1) if s.c1 else t["a0"]).to(dt)
    if s.ln_in:   # LayerNormalization of the stored bf16 rows, then the Dense
        x = F.layer_norm(x, (x.shape[-1],), gamma.to(dt), beta.to(dt), eps=1e-5)
    if s.ksize == 1 and s.stride == 1 and not s.upsample:
        y = x @ w[0, 0].to(dt)
    elif s.pad != s.pad_end:   # image_encoder.py PaddedConv2D(padding=((0,1),(0,1)))
        y = conv_ref(F.pad(x, (0, 0, s.pad, s.pad_end, s.pad, s.pad_end)), w.to(dt), None, stride=s.stride, pad=0)
    else:
        y = conv_ref(x, w.to(dt), None, stride=s.stride, pad=s.pad, upsample=s.upsample)
    del x
    if s.c2:   # shortcut operand: conv(h) + conv1x1(x)
        y += (torch.cat([t["a2"], t["a3"]], dim=-1) if s.c3 else t["a2"]).to(dt) @ wsc[0, 0].to(dt)
    if s.bias and not (s.split and s.ln_in):   # (a folded q|k|v projection has no bias of its own: only W beta)
        y += bias.to(dt)
    if s.rowvec:
        y += t["rv"][STEP].to(dt)[:, None, None, :]
    if s.act == ops.ACT_SILU:
        y = y * torch.sigmoid(y)
    elif s.act == ops.ACT_GEGLU:
        a, gate = y[..., :s.N // 2], y[..., s.N // 2:]
        y = a * 0.5 * gate * (1 + torch.tanh(gate * 0.7978845608 * (1 + 0.044715 * gate ** 2)))
    if s.residual:
        y += t["res"].to(dt)
    return y


def _packed(s, w, wsc, bias, gamma, beta, dev):
    """[N][K] bf16 weights as the engine's packers lay them (K = taps of the main operand, then the shortcut's channels; GEGLU
    rows interleaved; LayerNorm folded in) + the fp32 epilogue vectors, on the device."""
    from minsdtf_amd import packing

    wnk = w.permute(3, 0, 1, 2).reshape(s.N, -1)
    if wsc is not None:
        wnk = torch.cat([wnk, wsc.permute(3, 0, 1, 2).reshape(s.N, -1)], dim=1)
    b = bias if s.bias else None
    if _geglu(s):
        order = torch.from_numpy(packing.geglu_row_order(s.N // 2))
        wnk, b = wnk[order], (b[order] if b is not None else None)
    if s.ln_in:
        wf, cs, cb = packing.fold_layer_norm(wnk.contiguous(), None if s.split else b.numpy(), gamma.numpy(), beta.numpy(), dev)
        return wf, cb, cs
    return wnk.to(torch.bfloat16).contiguous().to(dev), (b.to(dev) if b is not None else None), None


def _row_moments(rows, slots):
    """Row-moment partials as a producing GEMM leaves them: (sum, sum of squares) of the stored bf16 row per column group."""
    C = rows.shape[-1]
    edges = [round(i * C / slots) for i in range(slots + 1)]
    return torch.stack([torch.stack([rows[:, a:b].sum(1), (rows[:, a:b] ** 2).sum(1)], -1) for a, b in zip(edges[:-1], edges[1:])], 1).float().contiguous()


@pytest.mark.parametrize("sig", list(CASES), ids=IDS)
def test_layer_launch(gpu, sig):
    """One recorded layer at every batch it was walked at.  Activations: bf16-rounded N(0.3, 1) (a non-zero mean, as the post-SiLU
    and post-GroupNorm tensors these layers read have), residual bf16 N(0, 1), weights N(0, 1) / sqrt(K) rounded to bf16, fp32
    bias and per-step row vector N(0, 1); sample i is seeded by (signature, i).  Bounds: close() of tests/test_ops_gpu.py as it
    stands (rtol 1e-2, atol 1e-2 max|ref|, relative RMS 2^-7 bf16 / 2^-12 fp32); atol 2e-2 max|ref| for the LayerNorm-fold
    consumers only, as test_conv_gemm_layer_norm_fold has it.  Then sample 0 and sample b - 1 of the batch-b launch carry the bits
    the same samples have in the largest batch."""
    from minsdtf_amd import ops, packing

    s, sid, dev = sig, LW.sig_id(sig), gpu
    per = CASES[s]
    Bmax = max(per)
    ho, wo = LW.out_hw(s)
    S, n_out = ho * wo, (s.N // 2 if _geglu(s) else s.N)
    f32 = s.out_dtype == ops.OUT_F32
    t = _draw(s, sid, Bmax)
    w, wsc, bias, gamma, beta = _weights(s, sid)
    ref = _reference(s, t, w, wsc, bias, gamma, beta).reshape(Bmax, S, n_out)
    wnk, bdev, colsum = _packed(s, w, wsc, bias, gamma, beta, dev)
    del w, wsc
    # every operand between guard bands (tests/_guard.py), sized by the header's extents (tests/_extents.py) for the batch it is launched
    # at; gw: what all batches share (weights, epilogue vectors, the step counter), g: one batch's activations and outputs
    geo0 = dict(h_in=s.h_in, w_in=s.w_in, c0=s.c0, c1=s.c1, c2=s.c2, c3=s.c3, N=s.N, ksize=s.ksize, stride=s.stride, upsample=s.upsample,
                pad=s.pad, pad_end=s.pad_end, act=s.act, out_dtype=s.out_dtype)
    gw = G.Guard(dev, X.conv_gemm(w=1, bias=bdev, ln_colsum=colsum, step_ptr=1, batch=1, **geo0))
    layouts = {0: gw.inp(wnk, "w")}
    bdev = None if bdev is None else gw.inp(bdev, "bias")
    colsum = None if colsum is None else gw.inp(colsum, "ln_colsum")
    step = gw.inp(torch.tensor([STEP], dtype=torch.int32), "step_ptr")
    d16 = {k: (v.to(torch.bfloat16) if (v is not None and k != "rv") else v) for k, v in t.items()}   # on the host: uploaded per batch
    atol = 2e-2 * float(ref.abs().max()) if s.ln_in else None
    sp = (S + 7) // 8 * 8          # V^T rows are read in 16-byte chunks
    ns2 = s.N - s.ns0 - s.ns1
    out_ld = max(s.ns0, 4)
    odt = torch.float32 if f32 else torch.bfloat16
    first = None                   # the largest batch's outputs, on the host
    for b in sorted(per, reverse=True):
        M = b * S
        geo = dict(batch=b, rv_step_stride=b * s.N if s.rowvec else 0, rv_batch_stride=s.N if s.rowvec else 0, **geo0)
        split_dims = (s.ns0, s.ns1, 1, s.ns1, 1, sp) if s.split else None
        g = G.Guard(dev, X.conv_gemm(a0=1, a1=d16["a1"], a2=d16["a2"], a3=d16["a3"], residual=d16["res"], rowvec=t["rv"], rv_steps=STEPS, **geo))
        d = {k: (g.inp(v[:b], {"res": "residual"}.get(k, k)) if (v is not None and k != "rv") else None) for k, v in d16.items()}
        rvd = g.inp(t["rv"][:, :b].contiguous(), "rowvec") if s.rowvec else None     # [STEPS][b][N]
        for l in per[b]:
            if l.w_layout not in layouts:
                layouts[l.w_layout] = gw.inp(packing.chunk_major(wnk) if l.w_layout == 1 else packing.fragment_major(wnk), "w", label=f"w layout {l.w_layout}")
            g.ext.update(X.conv_gemm(out=1, split=split_dims, out_ld=out_ld if s.split else None, workspace=1 if l.splitk > 1 else None, splitk=l.splitk,
                                     ln_in=1 if s.ln_in else None, ln_in_slots=l.ln_in_slots, ln_out=1 if s.ln_out else None,
                                     ln_out_slots=l.ln_out_slots, **geo))
            tag = f" {l.tile_m}x{l.tile_n} stages {l.stages} splitk {l.splitk} layout {l.w_layout}"
            ws = g.out((l.splitk * M, s.N), torch.float32, float("nan"), "workspace", label="workspace" + tag) if l.splitk > 1 else None
            kw = dict(a0=d["a0"], a1=d["a1"], a2=d["a2"], a3=d["a3"], w=layouts[l.w_layout], w_layout=l.w_layout,
                      bias=bdev, residual=d["res"], workspace=ws,
                      workspace_floats=0 if ws is None else ws.numel(), splitk=l.splitk, tile_m=l.tile_m, tile_n=l.tile_n, stages=l.stages, **geo)
            if s.rowvec:
                kw.update(rowvec=rvd, step_ptr=step)
            stats_in = stats_out = None
            if s.ln_in:
                stats_in = g.inp(_row_moments(t["a0"][:b].reshape(M, s.c0), l.ln_in_slots), "ln_in", label="ln_in" + tag)
                kw.update(ln_in=stats_in, ln_in_slots=l.ln_in_slots, ln_colsum=colsum, ln_eps=1e-5)
            if s.ln_out:
                assert l.ln_out_slots == ops.conv_gemm_ln_slots(N=s.N, tile_n=l.tile_n, tile_m=l.tile_m, ksize=s.ksize, act=s.act)
                stats_out = g.out((M, l.ln_out_slots, 2), torch.float32, float("nan"), "ln_out", label="ln_out" + tag)
                kw.update(ln_out=stats_out, ln_out_slots=l.ln_out_slots)
            if s.split:
                q = g.out((M, out_ld), torch.bfloat16, float("nan"), "out", label="q" + tag) if s.ns0 else None
                k = g.out((M, s.ns1), torch.bfloat16, float("nan"), "out1", label="k" + tag)
                vt = g.out((b, ns2, sp), torch.bfloat16, float("nan"), "out2", label="v^T" + tag)
                g.gaps(vt, S)      # columns [S, sp) of v^T are padding: a canary, not written
                kw.update(out=q, out_ld=out_ld, split=(s.ns0, s.ns1, k, s.ns1, vt, sp))
                outs = ([("q", q.view(b, S, -1), ref[:b, :, :s.ns0])] if s.ns0 else []) + \
                    [("k", k.view(b, S, s.ns1), ref[:b, :, s.ns0:s.ns0 + s.ns1]), ("v^T", vt[:, :, :S].permute(0, 2, 1), ref[:b, :, s.ns0 + s.ns1:])]
            else:
                out = g.out((M, n_out), odt, float("nan"), "out", label="out" + tag)
                kw.update(out=out)
                outs = [("out", out.view(b, S, n_out), ref[:b])]
            run_calls(ops.conv_gemm(**kw))
            what = f"{sid} | batch {b}{tag}"
            got = [(name, o.cpu().contiguous()) for name, o, _ in outs]
            for (name, o, r), (_, g_) in zip(outs, got):
                close(g_, r, atol=atol, what=f"{what} {name}")
            if stats_out is not None:   # the partials themselves: sum / sum of squares of the stored bf16 values
                tt, st = got[0][1].float().reshape(M, n_out), stats_out.cpu()
                assert torch.allclose(st[:, :, 0].sum(1), tt.sum(1), rtol=1e-4, atol=1e-2), f"{what}: row sums of the partials"
                assert torch.allclose(st[:, :, 1].sum(1), (tt * tt).sum(1), rtol=1e-4, atol=1e-2), f"{what}: row sums of squares of the partials"
            if first is None:
                first = got
            bits = torch.int32 if f32 else torch.int16
            for (name, g_), (_, g0) in zip(got, first):   # one numerics class per layer: a sample's bits do not depend on its batch
                for i in {0, b - 1}:
                    assert torch.equal(g_[i].view(bits), g0[i].view(bits)), f"{what} {name}: sample {i} differs from its bits at batch {Bmax}"
            g.check()
            del ws, kw, outs, got, stats_in, stats_out
        del g, d, rvd
    gw.check()
    _ran.add(sid)
    del t, d16, ref, layouts, wnk, first, gw
    gc.collect()
    torch.cuda.empty_cache()


def test_every_counted_case_ran(gpu):
    """No recorded signature is left out, skipped or deselected: the walk's count (kept by tests/test_layer_cases_cpu.py) is the
    number of cases that ran to their end in this session."""
    assert len(CASES) == LW.EXPECTED_CASES
    assert len(_ran) == LW.EXPECTED_CASES, sorted(set(IDS) - _ran)
