"""Diagnostics a caller can run on the tensors CodeFormer.forward returns (plain torch ops on the outputs: nothing here is on the hot path)."""
import torch


def top2_gap(logits):
    """Per-token gap between the largest and the second largest logit of a `(B, T, codebook)` tensor, and its minimum.

    The code index of a token is `argmax(logits)` (reference: `topk(softmax(logits), 1)`, codeformer_arch.py:257-258).  The HIP path reproduces
    the reference's logits to ~1e-5 (7e-6 on the goldens, tolerance 1e-4), so an index can only differ from the reference's where this gap is of
    that order.  The gate that admitted Winograd F(4x4,3x3) into the ENCODER (tests/test_gpu_real_images.py::test_encoder_logit_margin)
    was measured with seed-0 random-init weights -- the reference ships no checkpoint -- on seeded noise, the reference's real crops and
    synthetic range variants: smallest (gap / 2 x logit error) 7.0.  The network can act on this number itself: CodeFormer.logit_guard
    ('report' / 'rerun', CODEFORMER_HIP_LOGIT_GUARD) computes the same gap on the device in the argmax launch (cf_argmax_rows_gap, bitwise this
    function's values; `net.last_min_gap` is `gaps.min(dim=1)`) and runs the faces below `logit_guard_gap` (1.1e-4) again with the F(2x2,3x3)
    encoder.  This function stays the host-side statement of the rule, and what CPU tensors are measured with.
    Returns (gaps (B, T), min gap as a Python float)."""
    top = torch.topk(logits.detach().float(), 2, dim=-1).values
    gaps = top[..., 0] - top[..., 1]
    return gaps, float(gaps.min())
