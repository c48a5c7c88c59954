"""Host restatement (numpy) of the device generator of csrc/philox.h: the Philox4x32-10 block function, the counter layout and
the five derived kinds, written from the contract in include/pai_hip.h ("Device random numbers").  No device code.

    key     = (seed low 32 bits, seed high 32 bits)
    counter = (block, sub, stream, step)
    block   = flat element index // 4 (raw, uniform, normal, integer) or // 8 (keep bits)

The integer kinds are bit-exact restatements; the normal is computed in fp64 from the same integers (``normal`` also returns
the radius of each element's pair, which the device test's bound scales with)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF

STREAM_T, STREAM_U, STREAM_Z, STREAM_SAMPLER, STREAM_DROPOUT = 0, 1, 2, 3, 16
RAW, UNIFORM, NORMAL, INT, KEEP = 0, 1, 2, 3, 4


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints -> uint64 array [..., 4] holding the four 32-bit words."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK32) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    m32 = np.uint64(MASK32)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]                  # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & m32
        hi1, lo1 = p1 >> np.uint64(32), p1 & m32
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return np.stack(c, axis=-1)


def thr_of(p):
    """The 16-bit threshold of a dropout probability: round(p * 65536)."""
    return int(round(float(p) * 65536))


def blocks(nblocks, seed, sub, stream, step):
    """uint64 [nblocks, 4]: the words of the blocks 0 .. nblocks - 1 of the tuple."""
    if nblocks > 1 << 32:
        raise ValueError("more than 2^32 blocks")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    b = np.arange(nblocks, dtype=np.uint64)
    return philox4x32_10((b, int(sub), int(stream), int(step)), (seed & MASK32, seed >> 32))


def raw(n, seed, sub, stream, step):
    return blocks(-(-n // 4), seed, sub, stream, step).reshape(-1)[:n].astype(np.uint32)


def uniform(n, seed, sub, stream, step):
    """fp32 in [0, 1): (w >> 8) 2^-24, exact."""
    w = raw(n, seed, sub, stream, step)
    return ((w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def integer(n, T, seed, sub, stream, step):
    """int32 in [0, T): the high word of w * T."""
    w = raw(n, seed, sub, stream, step).astype(np.uint64)
    return ((w * np.uint64(T)) >> np.uint64(32)).astype(np.int32)


def keep(n, thr, seed, sub, stream, step):
    """uint8 0 / 1: eight per block, lane j = (w[j // 2] >> 16 (j % 2)) & 0xffff, kept iff lane >= thr."""
    w = blocks(-(-n // 8), seed, sub, stream, step)                 # [B, 4]
    lanes = np.stack([w & np.uint64(0xFFFF), (w >> np.uint64(16)) & np.uint64(0xFFFF)], axis=-1)   # [B, 4, 2]: j = 2 word + half
    return (lanes.reshape(-1)[:n] >= np.uint64(thr)).astype(np.uint8)


def normal(n, seed, sub, stream, step):
    """(z, r): fp64 standard normals of the n elements and the radius of each element's pair.  Words (w0, w1) -> (z0, z1) and
    (w2, w3) -> (z2, z3): u1 = ((wa >> 9) + 1) 2^-23, v = (wb >> 8) 2^-24, r = sqrt(-2 ln u1), z = r (cos 2 pi v, sin 2 pi v)."""
    w = blocks(-(-n // 4), seed, sub, stream, step).reshape(-1, 2)  # pairs
    u1 = ((w[:, 0] >> np.uint64(9)) + np.uint64(1)).astype(np.float64) * 2.0 ** -23
    v = (w[:, 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    z = np.stack([r * np.cos(2.0 * np.pi * v), r * np.sin(2.0 * np.pi * v)], axis=-1).reshape(-1)[:n]
    return z, np.repeat(r, 2)[:n]
