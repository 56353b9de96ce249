"""numpy restatement of the fp4 store's quantiser and decoder (include/phnsw.h): OCP MXFP4, blocks of 32 components,
e8 = clamp(floor(log2 maxabs) - 2 + 127, 2, 252) from the f32 exponent field, |x| * 2^(127 - e8) rounded to the E2M1
grid with ties to the even code, saturating at 6, no -0; decode = +-grid[code & 7] * 2^(e8 - 127).  All in f64, where
every product here is exact."""
import numpy as np

GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def quantize(rows):
    """rows [n, dim] f32 -> (codes [n, ceil(dim / 2)] u8, component j in nibble j & 1 of byte j >> 1; scales [n, ceil(dim / 32)] u8)"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, dim = rows.shape
    nb = (dim + 31) // 32
    x = np.zeros((n, nb, 32), dtype=np.float32)
    x.reshape(n, -1)[:, :dim] = rows
    field = (np.abs(x).max(axis=2).view(np.uint32) >> 23).astype(np.int64)
    e8 = np.clip(field - 2, 2, 252)
    y = np.ldexp(np.abs(x).astype(np.float64), (127 - e8)[:, :, None])
    mid, even_up = (GRID[:-1] + GRID[1:]) / 2, np.arange(1, 8) % 2 == 0  # a tie goes up exactly when the upper code is even
    mag = ((y[..., None] > mid) | ((y[..., None] == mid) & even_up)).sum(axis=-1)
    q = (np.where(mag > 0, np.signbit(x) * 8, 0) + mag).astype(np.uint8).reshape(n, nb * 32)[:, :dim + dim % 2]
    return (q[:, 0::2] | (q[:, 1::2] << 4)).astype(np.uint8), e8.astype(np.uint8)


def decode(codes, scales, dim):
    """what phnsw_store_read returns: [n, dim] f32"""
    q = np.stack([codes & 15, codes >> 4], axis=2).reshape(len(codes), -1)[:, :dim]
    v = np.where(q & 8, -1.0, 1.0) * GRID[q & 7]
    return np.ldexp(v, np.repeat(scales.astype(np.int64), 32, axis=1)[:, :dim] - 127).astype(np.float32)
