"""A PNG reader for the tests of buctd_amd.utils.vis.write_png: zlib and struct, nothing of the package."""
import struct
import zlib

import numpy as np


def decode_png(path):
    """8-bit RGB, non-interlaced, filter type 0 on every row -> uint8 [H, W, 3]; checks signature, CRCs and IHDR."""
    data = open(path, 'rb').read()
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    at, chunks = 8, []
    while at < len(data):
        n, = struct.unpack('>I', data[at:at + 4])
        tag, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        crc, = struct.unpack('>I', data[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(tag + body) & 0xffffffff, tag
        chunks.append((tag, body))
        at += 12 + n
    assert at == len(data)
    assert [t for t, _ in chunks] == [b'IHDR', b'IDAT', b'IEND']
    assert chunks[2][1] == b''
    w, h, depth, colour, compression, flt, interlace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert (depth, colour, compression, flt, interlace) == (8, 2, 0, 0, 0)
    raw = zlib.decompress(chunks[1][1])
    assert len(raw) == h * (1 + 3 * w)
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape(h, w, 3).copy()
