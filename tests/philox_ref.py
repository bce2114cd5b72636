"""numpy restatement of the device sampler's stream (include/phendiff_hip.h, pd_train_sample), written from the algorithm:
Philox4x32-10 in uint64 arithmetic, Box-Muller in float64, rounded to fp32 at the end.

    key     = (seed low 32 bits, seed high 32 bits)
    counter = (q low, q high, step low 32 bits, (step bits 32..47 << 16) | (rank << 4) | purpose)
    noise      flat element e: word e & 3 of counter q = e >> 2; words (0, 1) and (2, 3) are Box-Muller pairs with
               u = (x >> 8) 2^-24 + 2^-25, r = sqrt(-2 ln u_a), z_even = r cos(2 pi u_b), z_odd = r sin(2 pi u_b)
    timesteps  t_b = (x N) >> 32, x = word 0 of counter q = b under purpose 1

A plain module (no fixtures): imported by tests/test_host_train_sampler.py and tests/test_gpu_train_sampler.py."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
PURPOSE_NOISE, PURPOSE_TIMESTEPS, PURPOSE_RANDN = 0, 1, 2


def philox4x32_10(counter, key):
    """counter: four uint64 arrays (values < 2^32) of one shape, key: two Python ints -> four uint64 arrays (values < 2^32)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in counter)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    sh = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c0            # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c2
        n0 = (p1 >> sh) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> sh) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & MASK, n2, p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def _words(q, seed, step, rank, purpose):
    assert 0 <= rank < 4096 and 0 <= step < 1 << 48 and 0 <= purpose < 16
    q = np.asarray(q, dtype=np.uint64)
    c2 = np.full(q.shape, step & 0xFFFFFFFF, dtype=np.uint64)
    c3 = np.full(q.shape, (((step >> 32) & 0xFFFF) << 16) | (rank << 4) | purpose, dtype=np.uint64)
    return philox4x32_10((q & MASK, q >> np.uint64(32), c2, c3), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def _uniform(x):
    return (x >> np.uint64(8)).astype(np.float64) * 2.0 ** -24 + 2.0 ** -25


def normal(seed, step, rank, n, elem_base=0, purpose=PURPOSE_NOISE, with_radius=False):
    """n values of the noise stream from flat element `elem_base` on: float32 (float64 Box-Muller rounded once).  with_radius: also the
    float64 radius r of every element's pair (the scale of the parity bound)."""
    first, last = elem_base >> 2, (elem_base + n - 1) >> 2
    q = np.arange(first, last + 1, dtype=np.uint64)
    w = _words(q, seed, step, rank, purpose)
    z = np.empty((q.size, 4), dtype=np.float64)
    rad = np.empty((q.size, 4), dtype=np.float64)
    for a, b in ((0, 1), (2, 3)):
        r = np.sqrt(-2.0 * np.log(_uniform(w[a])))
        ang = 2.0 * np.pi * _uniform(w[b])
        z[:, a], z[:, b] = r * np.cos(ang), r * np.sin(ang)
        rad[:, a] = rad[:, b] = r
    lo = elem_base - 4 * first
    zf = z.reshape(-1)[lo:lo + n].astype(np.float32)
    return (zf, rad.reshape(-1)[lo:lo + n]) if with_radius else zf


def timesteps(seed, step, rank, B, N):
    """B timesteps in [0, N): int64."""
    x = _words(np.arange(B, dtype=np.uint64), seed, step, rank, PURPOSE_TIMESTEPS)[0]
    return ((x * np.uint64(N)) >> np.uint64(32)).astype(np.int64)
