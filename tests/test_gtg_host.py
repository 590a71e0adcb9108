"""Host side of `plot gtg` (no GPU): ERB row ratios and reshapes against the reference's golden values, the column edges of a
picture, the colour table, the formant mapping, the PNG writer, the command line and the ABI."""
import ctypes
import os
import re
import struct
import zlib

import numpy as np
import pytest

from conftest import ROOT
from f2cnn_amd import _lib, build, cli, png
from f2cnn_amd.scripts.plotting import PlottingProcessing as pp


@pytest.fixture(scope="module")
def golden_gtg():
    return np.load(os.path.join(ROOT, "tests", "golden", "f2cnn_golden_gtg.npz"))


@pytest.mark.parametrize("bank,height", [((16000, 128, 100), 941), ((16000, 64, 100), 466), ((16000, 8, 50), 54)])
def test_heights_and_ratios_are_the_reference_s(golden_gtg, bank, height):
    tag = "_".join(str(v) for v in bank)
    cf = golden_gtg["cf_" + tag]
    h, ratios = pp.GetNewHeightERB(np.zeros((bank[1], 3)), cf)
    assert h == height == int(golden_gtg["height_" + tag])
    assert ratios == golden_gtg["ratios_" + tag].tolist() and min(ratios) > 0
    assert all(type(r) is int for r in ratios)


def test_reshapes_are_the_reference_s_bit_for_bit(golden_gtg):
    cf, m = golden_gtg["cf_16000_8_50"], golden_gtg["reshape_matrix"]
    for got, want in ((pp.ReshapeEnvelopesForSpectrogram(m, cf), golden_gtg["reshape_whole"]),
                      (pp.ReshapeEnvelopesForSpectrogram(m, cf, start=5, end=30), golden_gtg["reshape_5_30"])):
        assert got.shape == want.shape and got.dtype == want.dtype == np.float64
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert golden_gtg["reshape_whole"].shape == (54, 37) and golden_gtg["reshape_5_30"].shape == (54, 25)


@pytest.mark.parametrize("m,W", [(1000, 7), (40, 64), (1, 1), (4099, 64)])
def test_column_edges_follow_the_definition(m, W):
    s = 11
    lo, hi = pp.column_edges(m, W, s)
    for x in range(W):
        want_lo, want_hi = s + (x * m) // W, s + ((x + 1) * m) // W
        if want_hi == want_lo:
            want_hi = want_lo + 1
        assert (lo[x], hi[x]) == (want_lo, want_hi)
    assert lo[0] == s and hi[-1] <= s + m and (hi > lo).all() and (lo >= s).all()
    if m >= W:      # bins tile the span without gap or overlap
        assert hi[-1] == s + m and (lo[1:] == hi[:-1]).all()
    else:           # every sample is shown, some more than once
        assert set(lo.tolist()) == set(range(s, s + m)) and (hi == lo + 1).all()


def test_colour_table():
    t = pp.colour_table()
    assert t.shape == (256, 3) and t.dtype == np.uint8
    assert t[0].tolist() == [255, 255, 255]
    assert t[1].tolist() == [0x44, 0x01, 0x54] and t[255].tolist() == [0xfd, 0xe7, 0x25]
    assert t[128].tolist() == [0x21, 0x91, 0x8c]                       # the middle anchor sits on a level
    assert (np.diff(t[1:, 1].astype(int)) >= 0).all()                   # green rises along the whole ramp
    # levels 64 and 65 straddle the second anchor (64.5): both within one step of it
    assert np.abs(t[64].astype(int) - [0x3b, 0x52, 0x8b]).max() <= 1 and np.abs(t[65].astype(int) - [0x3b, 0x52, 0x8b]).max() <= 1


def test_formant_mapping_at_the_corners():
    H, W, fs, low = 941, 300, 16000, 100
    start, end = 1000, 7000
    assert pp.formant_row(fs / 2, H, fs, low) == 0 and pp.formant_row(low, H, fs, low) == H - 1
    assert pp.formant_column(start, start, end, W) == 0
    assert pp.formant_column(end - 1, start, end, W) == W - 1 and pp.formant_column(end, start, end, W) == W
    assert pp.formant_column(start - 1, start, end, W) == -1
    assert pp.formant_row((fs / 2 + low) / 2, H, fs, low) == (H - 1) // 2
    # a track: frame j at sample 160 j; frames before `start` and after `end` are skipped, consecutive ones joined
    rgb = np.full((H, W, 3), 255, np.uint8)
    track = np.full(60, 4050.0)
    track[30:] = 2000.0
    drawn = pp.draw_formants(rgb, [track], 10000, fs, start, end, low)
    frames = [j for j in range(60) if start <= 160 * j < end]
    assert drawn == len(frames)
    black = np.flatnonzero((rgb == 0).all(axis=2).any(axis=0))
    assert black.tolist() == sorted({pp.formant_column(160 * j, start, end, W) for j in frames})
    r_hi, r_lo = pp.formant_row(4050.0, H, fs, low), pp.formant_row(2000.0, H, fs, low)
    col = pp.formant_column(160 * 30, start, end, W)                    # the jump: one vertical run
    assert (rgb[r_hi:r_lo + 1, col] == 0).all() and (rgb[r_hi - 1, col] == 255).all() and (rgb[r_lo + 1, col] == 255).all()


def decode_png(data):
    """8-bit truecolour, filter 0 only"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xffffffff
        chunks.append((kind, body))
        pos += 12 + n
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(b"".join(b for k, b in chunks if k == b"IDAT")), np.uint8).reshape(h, 1 + 3 * w)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(h, w, 3)


def test_write_png_round_trip(tmp_path):
    rgb = np.random.default_rng(5).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    path = pp.write_png(str(tmp_path / "a.png"), rgb)
    assert np.array_equal(decode_png(open(path, "rb").read()), rgb)
    assert np.array_equal(decode_png(png.png_bytes(rgb[:1, :1])), rgb[:1, :1])
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), rgb)
    with pytest.raises(ValueError):
        png.write_png(str(tmp_path / "b.png"), rgb.astype(np.float32))
    with pytest.raises(ValueError):
        png.write_png(str(tmp_path / "b.png"), rgb[:, :, :2])


def test_parser_takes_plot_gtg():
    a = cli.build_parser().parse_args(["plot", "gtg", "--file", "X", "--width", "300", "--pool", "max"])
    assert (a.plot_command, a.file, a.width, a.pool, a.all_files) == ("gtg", "X", 300, "max", False)
    assert (a.start, a.end, a.formant, a.CUTOFF, a.out) == (0, None, 5, None, None)
    b = cli.build_parser().parse_args(["plot", "gtg", "--all"])
    assert b.all_files is True and b.file is None and b.width == 1600 and b.pool == "mean"
    c = cli.build_parser().parse_args(["plot", "gtg", "-f", "X", "--cutoff", "50", "--formant", "2", "--start", "10", "--end", "90",
                                       "--out", "o.png"])
    assert (c.CUTOFF, c.formant, c.start, c.end, c.out) == (50, 2, 10, 90, "o.png")
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["plot", "gtg", "--all", "--file", "X"])
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["plot", "gtg", "--pool", "median"])
    assert "plot gtg" in cli.__doc__ and "organize" in cli.__doc__ and "plot_command" not in vars(
        cli.build_parser().parse_args(["cnn", "eval", "--file", "a.WAV"]))


def test_plot_gtg_without_a_file_says_so(capsys):
    assert cli.main(["plot", "gtg"]) == 1
    assert "--file" in capsys.readouterr().out


def test_abi_declares_the_picture_calls():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "f2cnn_hip.h")).read(), flags=re.S)
    for name in ("f2_envelope_picture", "f2_gammatonegram_batch"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["f2_envelope_picture"][1]) == 12 and len(_lib.SIGNATURES["f2_gammatonegram_batch"][1]) == 17
    lib = ctypes.CDLL(build.build_library())
    lib.f2_version.restype = ctypes.c_int
    assert lib.f2_version() >= 112
    assert hasattr(lib, "f2_envelope_picture") and hasattr(lib, "f2_gammatonegram_batch")
