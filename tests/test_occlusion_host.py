"""The host side of `cnn eval|evalnoise|evalrand --occlusion` (no GPU needed): the patch sets, the command line, the picture of
a synthetic map, the corpus table's weighting, and the three entries in header, library and ctypes table."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from f2cnn_amd import _lib, build, cli
from f2cnn_amd.scripts.CNN import Evaluating
from f2cnn_amd.scripts.plotting import PlottingCNN as pc
from f2cnn_amd.scripts.plotting.PlottingProcessing import colour_table
from test_gtg_host import decode_png


# ---- OcclusionPatches ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels,band,stride,count,last", [(128, 8, 8, 16, (120, 128)), (128, 16, 8, 15, (112, 128)),
                                                             (128, 10, 7, 18, (119, 128)), (5, 8, 8, 1, (0, 5))])
def test_channel_bands_counts_and_clipping(channels, band, stride, count, last):
    P = Evaluating.OcclusionPatches(11, channels, band, stride)
    assert P.dtype == np.int32 and P.shape == (count, 4)
    assert count == 1 + -(-max(channels - band, 0) // stride)
    assert (P[:, 0] == 0).all() and (P[:, 1] == 11).all()                      # all rows by default
    assert P[:, 2].tolist() == [i * stride for i in range(count)]
    assert (P[:-1, 3] - P[:-1, 2] == min(band, channels)).all() and tuple(P[-1, 2:]) == last
    covered = np.zeros(channels, bool)
    for _, _, c0, c1 in P:
        assert 0 <= c0 < c1 <= channels
        covered[c0:c1] = True
    assert covered.all()


def test_row_bands_are_the_major_order():
    P = Evaluating.OcclusionPatches(11, 128, 16, 8, 6, 5)
    assert P.shape == (2 * 15, 4)
    assert P[:15, :2].tolist() == [[0, 6]] * 15 and P[15:, :2].tolist() == [[5, 11]] * 15
    assert np.array_equal(P[:15, 2:], P[15:, 2:]) and np.array_equal(P[:15, 2:], Evaluating.OcclusionPatches(11, 128, 16, 8)[:, 2:])
    assert Evaluating.OcclusionPatches(11, 128, 128, 128, 4).tolist() == [[0, 4, 0, 128], [4, 8, 0, 128], [8, 11, 0, 128]]
    for bad in ((11, 128, 0, 8), (11, 128, 8, 0), (11, 0, 8, 8), (0, 128, 8, 8), (11, 128, 8, 8, 0), (11, 128, 8, 8, 3, 0)):
        with pytest.raises(ValueError):
            Evaluating.OcclusionPatches(*bad)


def test_the_occlusion_keyword_forms():
    spec = Evaluating._occlusion_spec
    assert spec(True) == dict(band=8, stride=8, row_band=None, row_stride=None, fill=0.0)
    assert spec((16, 4))["band"] == 16 and spec((16, 4))["stride"] == 4
    assert spec(dict(fill=0.5, row_band=3))["fill"] == 0.5 and spec(dict(row_band=3))["row_band"] == 3
    for bad in (dict(fill=1.5), dict(fill=-0.1), dict(fill=float("nan")), dict(bands=3)):
        with pytest.raises(ValueError):
            spec(bad)


# ---- the command line ----------------------------------------------------------------------------------------------------------
def parse(*argv):
    return cli.build_parser().parse_args(list(argv))


def test_the_flag_and_its_forms():
    for command in ("eval", "evalnoise", "evalrand"):
        args = parse("cnn", command, "-f", "X.WAV")
        assert "occlusion" not in vars(args) and "occlusion_rows" not in vars(args) and "occlusion_fill" not in vars(args)
        assert parse("cnn", command, "-f", "X.WAV", "--occlusion").occlusion == (8, 8)
        assert parse("cnn", command, "--occlusion", "-f", "X.WAV").occlusion == (8, 8)
        assert parse("cnn", command, "-f", "X.WAV", "--occlusion", "16").occlusion == (16, 16)
        assert parse("cnn", command, "-f", "X.WAV", "--occlusion", "16:4").occlusion == (16, 4)
    args = parse("cnn", "eval", "-f", "X.WAV", "--occlusion", "8:8", "--occlusion-rows", "6:5", "--occlusion-fill", "0.5", "--figure-width", "300")
    assert args.occlusion_rows == (6, 5) and args.occlusion_fill == 0.5 and args.figure_width == 300
    assert parse("cnn", "eval", "-f", "X.WAV", "--occlusion", "--occlusion-rows", "4").occlusion_rows == (4, 4)


@pytest.mark.parametrize("bad", ["0", "8:0", "-8", "8:", ":8", "8:8:8", "x", "8.5"])
def test_bad_forms_are_rejected(bad, capsys):
    with pytest.raises(SystemExit):
        parse("cnn", "eval", "-f", "X.WAV", "--occlusion=" + bad)
    with pytest.raises(SystemExit):
        parse("cnn", "eval", "-f", "X.WAV", "--occlusion", "--occlusion-rows=" + bad)
    capsys.readouterr()


def test_what_main_refuses(capsys):
    assert cli.main(["cnn", "noisesweep", "-f", "X.WAV", "--snrs", "3", "--occlusion"]) == 1
    assert "not supported" in capsys.readouterr().out
    assert cli.main(["cnn", "eval", "-f", "X.WAV", "--occlusion", "--occlusion-fill", "1.5"]) == 1
    assert "[0, 1]" in capsys.readouterr().out
    assert cli.main(["cnn", "eval", "-f", "X.WAV", "--occlusion-fill", "0.5"]) == 1
    assert "belong to --occlusion" in capsys.readouterr().out


def test_main_hands_the_flags_down(monkeypatch):
    seen = {}
    monkeypatch.setattr(Evaluating, "EvaluateOneWavFile", lambda **kw: seen.update(kw))
    assert not cli.main(["cnn", "eval", "-f", "X.WAV", "--occlusion", "16:8", "--occlusion-rows", "6:5", "--occlusion-fill", "0.25",
                         "--figure-width", "300"])
    assert seen["occlusion"] == dict(band=16, stride=8, row_band=6, row_stride=5, fill=0.25) and seen["figure_width"] == 300
    assert "figure" not in seen
    seen.clear()
    assert not cli.main(["cnn", "eval", "-f", "X.WAV"])
    assert "occlusion" not in seen and "figure_width" not in seen


# ---- the picture ---------------------------------------------------------------------------------------------------------------
def test_render_occlusion_on_a_synthetic_map(tmp_path):
    from f2cnn_amd.png import write_png
    C, W, K = 8, 12, 4
    ratios = [5, 4, 3, 3, 2, 2, 1, 1]
    H = sum(ratios)
    levels = np.full((C, W), 200, np.uint8)
    patches = Evaluating.OcclusionPatches(11, C, 2, 2)
    assert len(patches) == K
    m = np.zeros((K, W, 4))
    m[..., 0] = 3
    m[0, :, 2] = 0.5            # the top band raises P(rising) everywhere: the file's largest |mean d|
    m[1, :, 2] = -0.25          # the next lowers it, half as far
    m[2, :, 2] = 0.0            # no change
    m[3, :, 2] = np.linspace(-0.5, 0.5, W)
    m[:, 5, 0], m[:, 5, 2:] = 0, np.nan          # a column without rows
    rgb = pc.RenderOcclusion(levels, ratios, m, patches, (0, 1200), 16000)
    path = tmp_path / "occ.png"
    write_png(str(path), rgb)
    assert np.array_equal(decode_png(path.read_bytes()), rgb)
    assert rgb.shape == (2 * H + pc.GAP_ROWS, W, 3) and rgb.dtype == np.uint8
    assert (rgb[:H] == colour_table()[200]).all() and (rgb[H:H + pc.GAP_ROWS] == 255).all()       # gammatonegram, gap
    lower = rgb[H + pc.GAP_ROWS:]
    edges = np.concatenate([[0], np.cumsum(ratios)])
    band = lambda k: lower[edges[2 * k]:edges[2 * k + 2]]                      # the image rows of patch k's two channels
    others = [x for x in range(W) if x != 5]
    assert (band(0)[:, others] == np.array(pc.RED, np.uint8)).all()            # +scale: full red
    b1 = band(1)[0, 0].astype(int)
    assert b1[2] > b1[0] and (b1 != np.array(pc.BLUE)).any() and (b1 != 255).any()     # -scale / 2: bluish, between white and BLUE
    assert (np.abs(b1 - (255 + 0.5 * (np.array(pc.BLUE) - 255))) <= 1).all()
    assert (band(2)[:, others] == 255).all()                                   # no change: white
    assert (band(3)[:, 0] == np.array(pc.BLUE, np.uint8)).all() and (band(3)[:, W - 1] == np.array(pc.RED, np.uint8)).all()
    assert (lower[:, 5] == np.array(pc.GREY, np.uint8)).all()                  # the empty column, in every band
    # the ramp is symmetric about 0
    a, b = pc.diverging_colours(np.array([0.3]), 1.0)[0].astype(int), pc.diverging_colours(np.array([-0.3]), 1.0)[0].astype(int)
    assert np.abs((255 - a).sum() / (255 * 3 - sum(pc.RED)) - (255 - b).sum() / (255 * 3 - sum(pc.BLUE))) < 0.02
    # the formant's track stands on both panels
    flat = [1500.0] * 12
    drawn = pc.RenderOcclusion(levels, ratios, m, patches, (0, 1200), 16000, flat, 10000)
    black = (drawn == 0).all(axis=2)
    assert black[:H].any() and black[H + pc.GAP_ROWS:].any() and not black[H:H + pc.GAP_ROWS].any()
    assert np.array_equal(black[:H], black[H + pc.GAP_ROWS:])


def test_overlapping_bands_share_a_channel_by_their_mean():
    C, W = 4, 3
    patches = Evaluating.OcclusionPatches(11, C, 2, 1)       # [0,2) [1,3) [2,4)
    m = np.zeros((3, W, 4))
    m[..., 0] = 1
    m[0, :, 2], m[1, :, 2], m[2, :, 2] = 0.4, -0.4, 0.4
    rgb = pc.RenderOcclusion(np.ones((C, W), np.uint8), [1] * C, m, patches, (0, 30), 16000)
    lower = rgb[C + pc.GAP_ROWS:]
    assert (lower[0] == np.array(pc.RED, np.uint8)).all() and (lower[3] == np.array(pc.RED, np.uint8)).all()
    assert (lower[1] == 255).all() and (lower[2] == 255).all()                 # +0.4 and -0.4 meet: no net change


# ---- the corpus table ----------------------------------------------------------------------------------------------------------
def test_corpus_summary_sums_counts_and_weights_means_by_rows():
    a = np.array([[10, 2, 0.5, 0.6], [10, 0, -0.1, 0.1]])
    b = np.array([[30, 3, 0.1, 0.2], [30, 6, 0.3, 0.5]])
    none = np.array([[0, 0, np.nan, np.nan], [0, 0, np.nan, np.nan]])
    got = Evaluating.CombineOcclusionSummaries([a, none, b])
    assert got[:, 0].tolist() == [40, 40] and got[:, 1].tolist() == [5, 6]
    assert np.allclose(got[:, 2], [(10 * 0.5 + 30 * 0.1) / 40, (10 * -0.1 + 30 * 0.3) / 40], rtol=1e-15)
    assert np.allclose(got[:, 3], [(10 * 0.6 + 30 * 0.2) / 40, (10 * 0.1 + 30 * 0.5) / 40], rtol=1e-15)
    empty = Evaluating.CombineOcclusionSummaries([none, none])
    assert (empty[:, :2] == 0).all() and np.isnan(empty[:, 2:]).all()
    lines = Evaluating.OcclusionTable("all files", Evaluating.OcclusionPatches(11, 4, 2, 2), [[4000.0, 3000.0], [2000.0, 100.0]], got)
    assert len(lines) == 2 + 2 and "flips %" in lines[1] and "3000-4000" in lines[2].replace(" ", "") and "12.50" in lines[2]


# ---- the boundary --------------------------------------------------------------------------------------------------------------
def test_abi_declares_the_occlusion_calls():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "f2cnn_hip.h")).read(), flags=re.S)
    for name, nargs in (("f2_occlude_windows", 10), ("f2_occlusion_map", 12), ("f2_eval_occlusion_batch", 28)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    lib = ctypes.CDLL(build.build_library())
    for name in ("f2_occlude_windows", "f2_occlusion_map", "f2_eval_occlusion_batch"):
        assert hasattr(lib, name), name
    assert callable(_lib.Context.occlude_windows) and callable(_lib.Context.occlusion_map) and callable(_lib.Context.eval_occlusion_batch)
