"""Noise stream v1 restated in numpy from its definition (include/adx.h), not from the kernel.

    words    Philox4x32-10, key = (seed lo, seed hi), counter = (e >> 2, slot, tick lo, tick hi); element e takes w[e & 3]
    normals  u_i = ((w_i >> 8) + 0.5) * 2^-24;  r = sqrt(-2 ln u0), z0 = r cos(2 pi u1), z1 = r sin(2 pi u1); z2, z3 from
             (u2, u3); element e takes z[e & 3]

`normals(..., dtype=np.float64)` is the value the definition names; `dtype=np.float32` is the same formulas evaluated
step by step in fp32 with numpy's libm -- the yardstick for what an accurate fp32 implementation may lose.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
INIT_SLOT = 0xFFFFFFFF
_M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of 32-bit words, key: 2 -> the 4 output words as uint32 arrays."""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & _M32 for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & _M32, int(key[1]) & _M32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # 32 x 32 -> 64 bits, exact in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _M32, p1 >> np.uint64(32), p1 & _M32
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & _M32, (k1 + W1) & _M32
    return [v.astype(np.uint32) for v in c]


def _groups(seed, tick, slot, first, n):
    """The Philox outputs [4][groups] of the groups of four that cover the logical elements [first, first + n)."""
    g0, g1 = first >> 2, (first + n + 3) >> 2
    assert 0 <= first and g1 <= 1 << 32, "element index leaves the stream"
    ctr = (np.arange(g0, g1, dtype=np.uint64), int(slot) & _M32, int(tick) & _M32, (int(tick) >> 32) & _M32)
    return philox4x32_10(ctr, (int(seed) & _M32, (int(seed) >> 32) & _M32)), first - 4 * g0


def words(seed, tick, slot, first, n):
    w, skip = _groups(seed, tick, slot, first, n)
    return np.stack(w, axis=1).reshape(-1)[skip:skip + n]


def normals(seed, tick, slot, first, n, dtype=np.float64):
    w, skip = _groups(seed, tick, slot, first, n)
    f = dtype
    u = [((v >> np.uint32(8)).astype(f) + f(0.5)) * f(2.0 ** -24) for v in w]
    z = []
    for a, b in ((u[0], u[1]), (u[2], u[3])):
        r = np.sqrt(f(-2.0) * np.log(a))
        ang = f(2.0 * np.pi) * b
        z += [r * np.cos(ang), r * np.sin(ang)]
    out = np.stack(z, axis=1).reshape(-1)[skip:skip + n]
    assert out.dtype == dtype
    return out
