"""TEST INFRASTRUCTURE — NumPy restatement of the device noise source (``noise="device"``, edmp_amd/csrc/tail.h).

``philox4x32_10`` is Philox4x32-10 (Salmon et al. 2011, the Random123 constants) on uint64 arrays holding 32-bit words,
vectorised over the counter.  ``rng_normal8`` is tail.h's ``rng_normal8``: the same u32 words, ``u1`` / ``u2`` formed with the
kernel's float32 roundings, then the Box-Muller transform in float64 - an exact reference for everything but the kernel's own
float32 ``logf`` / ``sqrtf`` / ``sincospif``, whose error is a few float32 ulps.
"""
from __future__ import annotations

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)


def _u32(x):
    return np.asarray(x, dtype=np.uint64) & M32


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """four uint64 arrays of 32-bit words (broadcast together) for counter (c0, c1, c2, c3) and key (k0, k1)"""
    c0, c1, c2, c3 = np.broadcast_arrays(_u32(c0), _u32(c1), _u32(c2), _u32(c3))
    c0, c1, c2, c3 = c0.copy(), c1.copy(), c2.copy(), c3.copy()
    k0, k1 = _u32(k0), _u32(k1)
    for _ in range(10):
        p0 = PHILOX_M0 * c0  # < 2^64: exact in uint64
        p1 = PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def rng_normal8(seed: int, step: int, n_elem: int) -> np.ndarray:
    """(n_elem, 8) float64: the eight normals tail.h's rng_normal8(seed, step, elem) draws for elem = 0 .. n_elem-1.
    Counter (elem, step, blk, 0), key (low, high word of the 64-bit seed); z[4 blk + 2 h] = r cos(2 pi u2), z[4 blk + 2 h + 1] = r sin."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    elem = np.arange(n_elem, dtype=np.uint64)
    scale = np.float32(2.3283064365386963e-10)  # 2^-32
    z = np.empty((n_elem, 8))
    for blk in range(2):
        u = philox4x32_10(elem, int(step) & 0xFFFFFFFF, blk, 0, k0, k1)
        for h in range(2):
            u1 = (u[2 * h].astype(np.float32) + np.float32(1.0)) * scale  # (0, 1], float32 as the kernel rounds it
            u2 = u[2 * h + 1].astype(np.float32) * scale  # [0, 1)
            r = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
            a = 2.0 * np.pi * u2.astype(np.float64)
            z[:, 4 * blk + 2 * h] = r * np.cos(a)
            z[:, 4 * blk + 2 * h + 1] = r * np.sin(a)
    return z


def device_noise(seed: int, step: int, B: int, C: int, N: int) -> np.ndarray:
    """(B, C, N) float64 reference of Diffusion.device_noise(seed, step, B, C, N): element i = b N + l, channel c = z[i][c]."""
    z = rng_normal8(seed, step, B * N)[:, :C]
    return np.ascontiguousarray(z.reshape(B, N, C).transpose(0, 2, 1))
