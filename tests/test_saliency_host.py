"""The host side of `--saliency` (no GPU needed): the table from a hand-made summary, the corpus table's weighting, the picture of
a tiny map, and the three entries in header, library and ctypes table."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT
from f2cnn_amd import _lib, build
from f2cnn_amd.model import F2CNNModel
from f2cnn_amd.scripts.CNN import Evaluating
from f2cnn_amd.scripts.plotting import PlottingCNN as pc
from f2cnn_amd.scripts.plotting.PlottingProcessing import colour_table
from test_gtg_host import decode_png


# ---- the table -----------------------------------------------------------------------------------------------------------------
def test_table_from_a_hand_made_summary():
    cf = np.array([4000.0, 3000.0, 2000.0, 1000.0, 500.0])          # channel 0 the highest, as centre_freqs gives them
    summary = np.array([[40, 0.25, 0.5], [40, -0.125, 0.25], [40, 0.0, 0.125], [40, -0.5, 1.0], [40, 0.0625, 0.0625]])
    lines = Evaluating.SaliencyTable("X.WAV", cf, summary, 2)
    assert len(lines) == 2 + 3 and "X.WAV" in lines[0] and "2 channels" in lines[0]
    assert "sum G x" in lines[1] and "sum |G|" in lines[1] and "rows" in lines[1]
    cells = [line.split() for line in lines[2:]]
    assert [c[0] for c in cells] == ["3000-4000", "1000-2000", "500-500"]        # Hz ranges, low to high whatever the channel order
    assert [c[1] for c in cells] == ["0-1", "2-3", "4-4"]                         # the last band is clipped at the channel count
    assert [int(c[2]) for c in cells] == [40, 40, 40]
    assert [float(c[3]) for c in cells] == [0.125, -0.5, 0.0625]                  # sums over the band's channels, signed
    assert [float(c[4]) for c in cells] == [0.75, 1.125, 0.0625]
    assert cells[0][3].startswith("+") and cells[1][3].startswith("-")
    one = Evaluating.SaliencyTable("X.WAV", cf, summary, 8)                       # a band wider than the channels: one line
    assert len(one) == 3 and float(one[2].split()[3]) == summary[:, 1].sum()
    empty = Evaluating.SaliencyTable("X.WAV", cf, np.array([[0, np.nan, np.nan]] * 5), 5)
    assert int(empty[2].split()[2]) == 0 and "nan" in empty[2]


def test_corpus_summary_sums_rows_and_weights_means_by_rows():
    a = np.array([[10, 0.5, 0.6], [10, -0.1, 0.1]])
    b = np.array([[30, 0.1, 0.2], [30, 0.3, 0.5]])
    none = np.array([[0, np.nan, np.nan], [0, np.nan, np.nan]])
    got = Evaluating.CombineSaliencySummaries([a, none, b])
    assert got[:, 0].tolist() == [40, 40]
    assert np.allclose(got[:, 1], [(10 * 0.5 + 30 * 0.1) / 40, (10 * -0.1 + 30 * 0.3) / 40], rtol=1e-15)
    assert np.allclose(got[:, 2], [(10 * 0.6 + 30 * 0.2) / 40, (10 * 0.1 + 30 * 0.5) / 40], rtol=1e-15)
    empty = Evaluating.CombineSaliencySummaries([none, none])
    assert (empty[:, 0] == 0).all() and np.isnan(empty[:, 1:]).all()


# ---- the picture ---------------------------------------------------------------------------------------------------------------
def test_render_saliency_on_a_tiny_map(tmp_path):
    from f2cnn_amd.png import write_png
    C, W = 4, 12
    ratios = [5, 3, 2, 1]
    H = sum(ratios)
    levels = np.full((C, W), 200, np.uint8)
    m = np.zeros((C, W, 3))
    m[..., 0] = 3
    m[0, :, 1] = 0.5            # the top channel pushes P(rising) up everywhere: the file's largest magnitude
    m[1, :, 1] = -0.25          # the next pushes it down, half as far
    m[2, :, 1] = 0.0
    m[3, :, 1] = np.linspace(-0.5, 0.5, W)
    m[..., 2] = 9.0             # the |G| column is not drawn
    m[:, 5, 0], m[:, 5, 1:] = 0, np.nan          # a column without rows
    rgb = pc.RenderSaliency(levels, ratios, m, (0, 1200), 16000)
    path = tmp_path / "sal.png"
    write_png(str(path), rgb)
    assert np.array_equal(decode_png(path.read_bytes()), rgb)
    assert rgb.shape == (2 * H + pc.GAP_ROWS, W, 3) and rgb.dtype == np.uint8
    assert (rgb[:H] == colour_table()[200]).all() and (rgb[H:H + pc.GAP_ROWS] == 255).all()       # gammatonegram, gap
    lower = rgb[H + pc.GAP_ROWS:]
    edges = np.concatenate([[0], np.cumsum(ratios)])
    chan = lambda c: lower[edges[c]:edges[c + 1]]               # the image rows of channel c: ratios[c] of them
    assert [chan(c).shape[0] for c in range(C)] == ratios
    others = [x for x in range(W) if x != 5]
    assert (chan(0)[:, others] == np.array(pc.RED, np.uint8)).all()             # +scale: full red
    c1 = chan(1)[0, 0].astype(int)
    assert (np.abs(c1 - (255 + 0.5 * (np.array(pc.BLUE) - 255))) <= 1).all()     # -scale / 2: halfway from white to BLUE
    assert (chan(2)[:, others] == 255).all()                                    # nothing: white
    assert (chan(3)[:, 0] == np.array(pc.BLUE, np.uint8)).all() and (chan(3)[:, W - 1] == np.array(pc.RED, np.uint8)).all()
    assert (lower[:, 5] == np.array(pc.GREY, np.uint8)).all()                   # the empty column, in every channel
    # an all-empty map (an utterance too short for a window) is grey below its picture
    none = np.zeros((C, W, 3))
    none[..., 1:] = np.nan
    assert (pc.RenderSaliency(levels, ratios, none, (0, 1200), 16000)[H + pc.GAP_ROWS:] == np.array(pc.GREY, np.uint8)).all()
    # the formant's track stands on both panels
    drawn = pc.RenderSaliency(levels, ratios, m, (0, 1200), 16000, [1500.0] * 12, 10000)
    black = (drawn == 0).all(axis=2)
    assert black[:H].any() and black[H + pc.GAP_ROWS:].any() and not black[H:H + pc.GAP_ROWS].any()
    assert np.array_equal(black[:H], black[H + pc.GAP_ROWS:])


# ---- the boundary --------------------------------------------------------------------------------------------------------------
def test_abi_declares_the_saliency_calls():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "f2cnn_hip.h")).read(), flags=re.S)
    for name, nargs in (("f2_cnn_input_gradient", 8), ("f2_saliency_map", 11), ("f2_eval_saliency_batch", 25)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    lib = ctypes.CDLL(build.build_library())
    for name in ("f2_cnn_input_gradient", "f2_saliency_map", "f2_eval_saliency_batch"):
        assert hasattr(lib, name), name
    assert callable(_lib.Context.cnn_input_gradient) and callable(_lib.Context.saliency_map) and callable(_lib.Context.eval_saliency_batch)
    assert callable(F2CNNModel.input_gradient)
    assert lib.f2_version() == 115      # (114 until f2_cnn_layers: the saliency calls came without a new number)
