"""A PNG writer for the pictures of `plot gtg`: 8-bit truecolour, no interlace, filter 0 on every row. zlib and struct
only - matplotlib and PIL are not dependencies of this package."""
import struct
import zlib

import numpy

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload) & 0xffffffff)


def png_bytes(rgb, level=6):
    rgb = numpy.ascontiguousarray(rgb)
    if rgb.dtype != numpy.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.shape[0] < 1 or rgb.shape[1] < 1:
        raise ValueError("write_png takes an (H, W, 3) uint8 array with H, W >= 1")
    h, w = rgb.shape[:2]
    rows = numpy.zeros((h, 1 + 3 * w), numpy.uint8)          # every row: filter type 0, then its RGB bytes
    rows[:, 1:] = rgb.reshape(h, 3 * w)
    return b"".join((SIGNATURE,
                     _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)),
                     _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)),
                     _chunk(b"IEND", b"")))


def write_png(path, rgb):
    """Write the (H, W, 3) uint8 array `rgb` as an 8-bit truecolour PNG."""
    data = png_bytes(rgb)
    with open(path, "wb") as f:
        f.write(data)
    return path
