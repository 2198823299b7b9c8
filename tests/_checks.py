"""The comparison helpers of the kernel tests, shared by GPU and CPU test modules (plain torch, no device needed).  Not a conftest:
imported by name."""
import torch


def bf(x):
    """Round an fp32 CPU tensor to bf16 and back (what the device will see)."""
    return x.to(torch.bfloat16).to(torch.float32)


def close(got, ref, rtol=1e-2, atol=None, what="", rms=None):
    """Element-wise: |got - ref| <= atol + rtol |ref| everywhere.  Aggregate: relative RMS error ||got - ref|| / ||ref|| <=
    `rms`, by default 2^-7 for a bf16 result (its own rounding is 2^-9 relative per element) and 2^-12 for an fp32 result of
    bf16 operands — the element-wise floor alone would let a dropped K chunk of one tap of a K = 2,304 contraction through;
    the aggregate does not."""
    is_f32 = got.dtype == torch.float32
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    if atol is None:
        atol = 1e-2 * float(ref.abs().max()) + 1e-6
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())}/{got.numel()} non-finite outputs"
    err = (got - ref).abs()
    bad = err > (atol + rtol * ref.abs())
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} mismatches, max err {float(err.max()):.4g}, ref max {float(ref.abs().max()):.4g}"
    if rms is None:
        rms = 2.0 ** -12 if is_f32 else 2.0 ** -7
    rel = float((got - ref).double().norm() / max(float(ref.double().norm()), 1e-30))
    assert rel <= rms, f"{what}: relative RMS error {rel:.3g} > {rms:.3g}"
