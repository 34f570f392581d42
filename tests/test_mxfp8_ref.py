"""The reference MXFP8 quantiser (tests/mxfp8_ref.py) against values worked out by hand from the format's definition."""
import numpy as np

import mxfp8_ref as R


def block(**at):
    v = np.zeros((1, 32), np.float32)
    for i, x in at.items():
        v[0, int(i[1:])] = x
    return v


def test_edge_blocks():
    q, s = R.quantize(block())                                         # all zeros: e = -127
    assert s[0, 0] == 0 and not q.any()
    q, s = R.quantize(block(k0=8.0, k1=-1.0, k2=0.0))                  # amax = 2^3: e = -5, 8 -> 256 = 0x78, -1 -> -32 = 0xE0
    assert s[0, 0] == 122 and (q[0, 0], q[0, 1], q[0, 2]) == (0x78, 0xE0, 0x00)
    q, s = R.quantize(block(k0=np.float32(1.0) - np.float32(2.0 ** -24)))   # just under one: e = -9, scaled just under 512 -> clamped to 448 = 0x7E
    assert s[0, 0] == 118 and q[0, 0] == 0x7E
    q, s = R.quantize(block(k0=480.0, k1=-500.0, k2=449.0, k3=464.0, k4=17.0))   # e = 0; beyond 448: clamped, never the NaN byte; 17 -> 16 (tie to even)
    assert s[0, 0] == 127 and list(q[0, :5]) == [0x7E, 0xFE, 0x7E, 0x7E, 0x58]
    q, s = R.quantize(block(k0=2.0 ** -130))                           # below 2^-118: e clamps to -127, the element is 2^-3
    assert s[0, 0] == 0 and q[0, 0] == 0x20


def test_dequantize_and_idempotence():
    x = R.edge_rows()
    q, s = R.quantize(x)
    y = R.dequantize(q, s)
    amax = np.abs(x).reshape(8, -1, 32).max(axis=2).repeat(32, axis=1)
    assert np.all(np.abs(y - x) <= 2.0 ** -4 * np.abs(x) + 2.0 ** -9 * amax + (np.abs(x) > 0.875 * amax) * 0.125 * amax)   # half a step, or the clamp
    q2, s2 = R.quantize(y)
    assert np.array_equal(q2, q) and np.array_equal(s2, s) and np.array_equal(R.dequantize(q2, s2), y)
