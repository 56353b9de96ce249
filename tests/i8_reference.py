"""numpy restatement of the i8 store's quantiser (include/phnsw.h): per row and symmetric,
scale = maxabs / 127 and code = clamp(rint(x / scale), -127, 127), both divisions in IEEE f32; a scale of 0 (a row
of zeros, or a maxabs so small that maxabs / 127 underflows to 0) gives codes 0."""
import numpy as np


def quantize(rows):
    """rows [n, dim] f32 -> (codes [n, dim] int8, scales [n] f32)"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    scales = (np.abs(rows).max(axis=1) / np.float32(127.0)).astype(np.float32)
    safe = np.where(scales > 0, scales, np.float32(1.0)).astype(np.float32)
    with np.errstate(over="ignore"):
        t = np.rint((rows / safe[:, None]).astype(np.float32))  # round half to even, as rintf
    codes = np.clip(t, -127.0, 127.0).astype(np.int8)
    codes[scales == 0] = 0
    return codes, scales


def dequantize(codes, scales):
    """what phnsw_store_read returns: scale * (float)code, one f32 multiply"""
    return (scales[:, None].astype(np.float32) * codes.astype(np.float32)).astype(np.float32)
