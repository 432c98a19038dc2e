"""Shared by the scoring tests: the error bound of a log-softmax row and the reference's masked-marginal loop."""
import torch


def ulp32(v):
    """Spacing of fp32 at |v| (a float64 tensor): 2^(floor(log2 |v|) - 23)."""
    v = v.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(v)) - 23)


def row_bound(ref):
    """[n] bounds for fp32 log-softmax rows against ``ref`` [n, V] (fp64 log_softmax of the same fp32 logits): 4 fp32 ulp at
    the largest |reference value| of the row — one rounding each for the max-shift x - max, the sum of the exponentials
    (its relative error is an absolute error of the log), the log and the final subtraction; every one of them is at most
    an ulp of a value no larger than the row's largest |log-probability| (which is >= log V > 2)."""
    return 4 * ulp32(ref.abs().amax(-1))


def check_rows(got, logits32, what=""):
    """got fp32 [n, V] against log_softmax of the fp32 ``logits32`` taken in fp64; prints the figure, then asserts."""
    ref = torch.log_softmax(logits32.double().cpu(), -1)
    err = (got.double().cpu() - ref).abs().amax(-1)
    bound = row_bound(ref)
    print(f"\n{what}: max err / bound = {(err / bound).max().item():.3f} (max err {err.max().item():.3e}, {got.shape[0]} rows)")
    assert torch.isfinite(got).all()
    assert (err <= bound).all(), (what, (err / bound).max().item())
    return ref


def masked_loop_logits(model, tokens):
    """The reference's masked-marginal loop (examples/variant-prediction/predict.py:205-215) on this model's own forward at
    B = 1, for every sequence of the padded batch and every non-pad position: fp32 logits [B, T, V] of the masked row
    (zero on <pad> rows).  ``tokens`` on the device."""
    B, T = tokens.shape
    out = torch.zeros((B, T, model.alphabet_size), dtype=torch.float32, device=tokens.device)
    host = tokens.cpu()
    with torch.no_grad():
        for b in range(B):
            for i in range(T):
                if host[b, i].item() == model.padding_idx:
                    continue
                masked = tokens[b:b + 1].clone()
                masked[0, i] = model.mask_idx
                out[b, i] = model(masked)["logits"][0, i].float()
    return out
