"""A numpy restatement of the channels_last packed format (include/cnnq_hip.h), written from the format's
words alone: row r of [R][C] is one little-endian bit stream, channel c at bits [coloff[c], coloff[c] + bits[c]), coloff the
exclusive prefix sum of the widths, every row padded with zero bits to whole dwords."""
import numpy as np


def coloff(bits):
    bits = np.asarray(bits, dtype=np.int64)
    assert bits.ndim == 1 and ((bits >= 0) & (bits <= 8)).all()
    return np.concatenate([[0], np.cumsum(bits)]).astype(np.int64)


def rowbytes(bits):
    return 4 * ((int(coloff(bits)[-1]) + 31) // 32)


def pack(codes, bits):
    """codes [R, C] (integers; only the low bits[c] bits of a code enter the stream) -> the buffer's R * rowbytes bytes."""
    codes = np.asarray(codes).astype(np.int64)
    R, C = codes.shape
    off = coloff(bits)
    assert len(off) == C + 1
    nbits = 8 * rowbytes(bits)
    stream = np.zeros((R, nbits), dtype=np.uint8)                     # one entry per bit of a row, bit i of the row at [i]
    for c in range(C):
        for k in range(int(bits[c])):
            stream[:, off[c] + k] = (codes[:, c] >> k) & 1
    # bit i of a row is bit i % 8 of byte i // 8: little-endian within the byte, bytes in ascending order
    return np.packbits(stream.reshape(R, nbits // 8, 8), axis=-1, bitorder='little').reshape(-1).tobytes() if nbits else b''


def unpack(buf, bits, R, C):
    """the buffer's bytes -> codes [R, C] (int64)"""
    off = coloff(bits)
    assert len(off) == C + 1
    rb = rowbytes(bits)
    raw = np.frombuffer(bytes(buf), dtype=np.uint8)
    assert raw.size == R * rb, (raw.size, R, rb)
    codes = np.zeros((R, C), dtype=np.int64)
    if rb == 0:
        return codes
    stream = np.unpackbits(raw.reshape(R, rb), axis=-1, bitorder='little').astype(np.int64)
    for c in range(C):
        for k in range(int(bits[c])):
            codes[:, c] |= stream[:, off[c] + k] << k
    return codes
