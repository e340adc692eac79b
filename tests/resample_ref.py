"""Float64 restatement of the GPU sinc resampler (csrc/resample.hip) for tests/test_gpu_resample_matrix.py.

The kernel's own statement, summed directly in float64 for any filter bank kern[new][K]:

    y[o] = sum_{m < K} kern[k][m] * x[j * orig + m - width],   o = j * new + k,   x = 0 outside [0, L)

(tests/test_ingest.py test_oracle_resampler_against_direct_float64 holds the same loop for the torchaudio filters),
and the same sum as oracle/resample_oracle.resample forms it (pad, conv1d(stride = orig), interleave the phases) in
float32 for a filter bank that is not torchaudio's.  TEST INFRASTRUCTURE ONLY."""

import numpy as np
import torch
import torch.nn.functional as F

RS_MAX_KERN = 32768  # csrc/resample.hip: filter banks of up to this many floats are staged in LDS


def takes_lds_kernel(new: int, taps: int) -> bool:
    """Which of the two kernels resample_sinc_launch picks: resample_sinc_kernel<true> (filters in LDS) or <false>."""
    return new * taps <= RS_MAX_KERN


def out_len(n: int, orig: int, new: int) -> int:
    return -(-new * n // orig)


def direct64(x: np.ndarray, kern: np.ndarray, orig: int, width: int, lout: int) -> np.ndarray:
    """x (B, L), kern (new, K) -> (B, lout) float64."""
    x = np.asarray(x, np.float64)
    kern = np.asarray(kern, np.float64)
    B, L = x.shape
    new, K = kern.shape
    nj = -(-lout // new)
    xp = np.zeros((B, max(width + L, (nj - 1) * orig + K) + 1))
    xp[:, width:width + L] = x
    y = np.empty((B, nj, new))
    for j in range(nj):
        y[:, j] = xp[:, j * orig:j * orig + K] @ kern.T
    return y.reshape(B, nj * new)[:, :lout]


def conv32(x: torch.Tensor, kern: torch.Tensor, orig: int, width: int, lout: int) -> torch.Tensor:
    """The float32 oracle's formulation (oracle/resample_oracle.resample) for any filter bank kern (new, K)."""
    new, K = kern.shape
    nj = -(-lout // new)
    right = max(0, (nj - 1) * orig + K - width - x.shape[1])
    y = F.conv1d(F.pad(x, (width, right))[:, None], kern[:, None], stride=orig)
    return y.transpose(1, 2).reshape(x.shape[0], -1)[:, :lout]


def lin_for_lout(target: int, orig: int, new: int) -> int:
    """The smallest input length whose output has at least `target` samples."""
    n = 1
    while out_len(n, orig, new) < target:
        n += 1
    return n
