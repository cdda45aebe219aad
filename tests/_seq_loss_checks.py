"""The bounds of the sequence, loss and spectral-norm kernels' fp64 tests (not collected by pytest). tests/test_seq_loss_fp64_gpu.py (through
ops) and tests/test_seq_loss_abi_fp64_gpu.py (at the C ABI) hold the same kernels to them; tests/test_seq_loss_ref_cpu.py and
tests/test_abi_cases_cpu.py seed their flaws against them."""
from oracle import abi_cases as AC

ULP = 2.0 ** -23
# (relative L2, max|err| / max|ref|), derived: the expected value is an fp64-exact quantity rounded to fp32 once, or twice where noted
DERIVED = {
    # sum of fp32 terms in double, then one rounding of the mean: |a - b|, 1 - a, 1 + a are each one fp32 rounding of an exact difference
    # (non-negative terms: the sum keeps the relative error of its terms), the mean of a itself has exact terms
    "loss_value": (ULP, ULP),
    # (a - b)^2: the difference and its square are rounded, then the mean: one more ulp
    "loss_value_mse": (2 * ULP, 2 * ULP),
    # +-float(gout * scale / n): scale / n is rounded once, gout = 0.5 is a power of two
    "loss_grad_const": (ULP, ULP),
}
# (relative L2, max|err| / max|ref|) per family: 4x the worst case measured on an MI355X (in brackets), rounded down to two digits.
# The flaws tests/test_seq_loss_ref_cpu.py seeds move some case of the family concerned by 10x its bound or more.
BOUNDS = {
    "lsm_fwd": (2.1e-7, 4.3e-7),          # [5.3e-8, 1.1e-7]
    "lsm_grad": (7.9e-6, 2.3e-5),         # [2.0e-6, 5.8e-6]  (the 30 x randn + 60 logits: log-probs near -200 carry an absolute error of 1e-5 into exp)
    "ctc_plain_loss": (7.3e-7, 7.3e-7),   # [1.8e-7, 1.8e-7]  unit-variance logits
    "ctc_plain_grad": (2.5e-4, 6.4e-4),   # [6.3e-5, 1.6e-4]  d log-probs and d logits; torch's fp32 ctc_loss: 4.2e-5 on the same case
    "ctc_peaked_loss": (4.6e-7, 4.6e-7),  # [1.2e-7, 1.2e-7]  peaked logits, 3 x randn over 281 states
    "ctc_peaked_grad": (1.6e-3, 3.1e-3),  # [4.0e-4, 7.9e-4]  torch's fp32 ctc_loss: 4.0e-4
    "ctc_long_loss": (1.6e-6, 1.6e-6),    # [4.0e-7, 4.0e-7]  600 steps of 4 x randn
    "ctc_long_grad": (1.1e-2, 2.2e-2),    # [2.8e-3, 5.6e-3]  torch's fp32 ctc_loss: 2.8e-3
    "mse_grad": (2.8e-7, 6.7e-7),         # [7.0e-8, 1.7e-7]
    "sn_uv": (1.2e-6, 1.9e-6),            # [3.0e-7, 4.8e-7]  persisted u, v after one and after two iterations
    "sn_sigma": (4.2e-7, 4.2e-7),         # [1.1e-7, 1.1e-7]  sigma and 1 / sigma
    "sn_w": (4.3e-7, 5.1e-7),             # [1.1e-7, 1.3e-7]
    "sn_grad": (5.0e-7, 6.4e-7),          # [1.3e-7, 1.6e-7]  returned and added to a pre-filled parameter gradient
    "pixelnorm_fwd": (2.2e-7, 4.6e-7),    # [5.6e-8, 1.2e-7]
    "pixelnorm_grad": (2.2e-7, 3.8e-7),   # [5.7e-8, 9.7e-8]
    # one channel: y = x / sqrt(x^2 + eps) is +-1 and dx = dy eps / (x^2 + eps)^1.5 is 1e-8 of the two terms dy / d and x^2 dy / d^3 it is the
    # difference of - no fp32 evaluation keeps a digit of it. The error is measured against those terms (max |dy / d|), not against dx.
    "pixelnorm_grad_c1": (2.3e-7, 2.5e-7),  # [5.8e-8, 6.4e-8]
}


def _leaf(t):
    return t.double().clone().requires_grad_(True)


ACC_CASES = [c for c in AC.LOSS_CASES if c[2] in (255, 4097)]          # the loss cases the accumulate = 1 calls run at
