"""Host side of `cnn eval --figure` (no GPU): the value axis, the formant's slope track against a per-window lstsq / pearsonr
loop, the glyph table, the pixels of a hand-made figure at their computed positions, the command line and the ABI."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
from scipy.stats import pearsonr

import label_referee as lr
from conftest import ROOT
from f2cnn_amd import _lib, build, cli
from f2cnn_amd.scripts.plotting import PlottingCNN as pc
from f2cnn_amd.scripts.plotting import PlottingProcessing as pp
from f2cnn_amd.scripts.processing.FBFileReader import GetFormantFrequencies


def test_value_row_spans_the_reference_s_axis():
    assert [pc.value_row(y, 321) for y in (-1.6, 0, 0.5, 1, 1.6)] == [320, 160, 110, 60, 0]
    assert pc.value_row(0.0, 33) == 16 and pc.LOWER_ROWS == 321


def test_formant_slope_track_against_lstsq_and_pearsonr(tmp_path):
    wav = lr.write_labelled_file(tmp_path, lambda n: np.zeros(n, np.int16))
    track, period = GetFormantFrequencies(os.path.splitext(wav)[0] + ".FB", 2)
    radius, spf = 5, 16000 * period / 1e6
    positions, angle, p = pc.FormantSlopeTrack(track, radius, spf)
    centres = range(radius, len(track) - radius)                    # every frame with a whole window, the last one included
    assert len(centres) == 125 - 2 * radius and np.array_equal(positions, np.array(centres) * spf) and spf == 160.0
    for i, k in enumerate(centres):
        y = track[k - radius:k + radius + 1]
        x = np.arange(k - radius, k + radius + 1) * spf
        (a, b), _, _, _ = np.linalg.lstsq(np.vstack([x, np.ones(len(x))]).T, y, rcond=None)
        assert abs(np.tan(angle[i]) - a) <= 1e-12 * abs(a), (k, np.tan(angle[i]), a)      # solver round-off
        assert abs(p[i] - pearsonr(y, a * x + b)[1]) <= 1e-9, k
    assert angle.min() < 0 < angle.max()                             # the sinusoid rises and falls
    short = pc.FormantSlopeTrack(track[:2 * radius], radius, spf)
    assert all(len(part) == 0 for part in short)


def test_text_mask_glyphs():
    chars = "abcdefghijklmnopqrstuvwxyz0123456789#-.:% "
    assert sorted(pc.GLYPHS) == sorted(chars)
    assert pc.text_mask("ax-h").shape == (7, 23) and pc.text_mask("q").shape == (7, 5) and pc.text_mask("").shape == (7, 0)
    assert pc.text_mask("h#").dtype == bool
    for ch in chars:
        assert pc.GLYPHS[ch].shape == (7, 5)
        assert pc.GLYPHS[ch].any() == (ch != " "), ch                 # (the space is the one empty glyph)
    for a, b in itertools.combinations(chars, 2):
        assert not np.array_equal(pc.GLYPHS[a], pc.GLYPHS[b]), (a, b)
    two = pc.text_mask("A1")                                          # capitals are folded; one empty column between glyphs
    assert np.array_equal(two[:, :5], pc.GLYPHS["a"]) and not two[:, 5].any() and np.array_equal(two[:, 6:], pc.GLYPHS["1"])
    with pytest.raises(KeyError):
        pc.text_mask("é")


W, RATIOS, RATE = 40, [3, 2, 1], 16000
SPAN = (0, 4000)                                                      # 100 samples per column


def hand_track():
    """columns 0-9 rising only, 10-19 falling only, 20-24 both, 25-29 empty, 30-39 rising only"""
    t = np.full((W, 5), np.nan)
    t[:, :2] = 0
    for x in itertools.chain(range(0, 25), range(30, 40)):
        rising = 4 if x < 10 or x >= 30 else 0 if x < 20 else 2
        t[x] = (4, rising, 0.25 + 0.5 * (x % 2), 0.1, 0.9)
    return t


def render(**kw):
    levels = np.array([[1] * W, [128] * W, [255] * W], np.uint8)
    levels[1, 7] = 0                                                  # a masked pixel
    return pc.RenderFigure(levels, RATIOS, hand_track(), SPAN, RATE, **kw), levels


def test_render_figure_pixels():
    rgb, levels = render(phonemes=[("aa", 0, 1650), ("h#", 1650, 3999)], accuracy=0.75)
    h1 = sum(RATIOS)
    assert rgb.shape == (h1 + pc.GAP_ROWS + pc.LOWER_ROWS + pc.STRIP_ROWS, W, 3) and rgb.dtype == np.uint8
    table = pp.colour_table()
    # upper panel: ticks of 9 rows centred on 2500 / 500 Hz are taller than this 6-row picture and clip to it
    r_rise, r_fall = pp.formant_row(2500, h1, RATE, 100), pp.formant_row(500, h1, RATE, 100)
    assert (r_rise, r_fall) == (3, 5)
    assert tuple(rgb[r_rise, 3]) == pc.RED and tuple(rgb[r_fall, 3]) == pc.RED and tuple(rgb[0, 3]) == pc.RED   # rows -1 .. 5: all six
    assert tuple(rgb[r_fall, 12]) == pc.BLUE and tuple(rgb[0, 12]) == tuple(table[1])                            # blue: rows 1 .. 5
    assert tuple(rgb[1, 22]) == pc.BLUE                                # both: the falling tick is drawn last
    assert np.array_equal(rgb[:h1, 27], table[np.repeat(levels[:, 27], RATIOS)])                               # neither
    assert tuple(rgb[0, 27]) == tuple(table[1]) and tuple(rgb[5, 27]) == tuple(table[255])
    assert (rgb[h1:h1 + pc.GAP_ROWS] == 255).all()
    lower = rgb[h1 + pc.GAP_ROWS:h1 + pc.GAP_ROWS + pc.LOWER_ROWS]
    row = lambda y: pc.value_row(y, pc.LOWER_ROWS)
    # the mean curve: 0.25 in even columns, 0.75 in odd ones, joined by a vertical run in the later column
    assert tuple(lower[row(0.25), 2]) == pc.BLUE and tuple(lower[row(0.75), 3]) == pc.BLUE
    assert tuple(lower[row(0.5), 3]) == pc.BLUE                        # the run up to 0.75 crosses the grey line in column 3 ...
    assert tuple(lower[row(0.5), 0]) == pc.LIGHT_BLUE                  # ... which the band covers in column 0, where no run starts
    assert tuple(lower[row(0.5), 27]) == pc.GREY and tuple(lower[row(0.0), 5]) == pc.GREY and tuple(lower[row(1.0), 5]) == pc.GREY
    assert tuple(lower[row(0.9), 2]) == pc.LIGHT_BLUE and tuple(lower[row(0.1), 2]) == pc.LIGHT_BLUE
    assert tuple(lower[row(0.9) - 1, 2]) == pc.WHITE and tuple(lower[row(0.1) + 1, 2]) == pc.WHITE
    # an empty column shows neither band nor curve, and the curve starts anew behind it (no run in column 30)
    for x in range(25, 30):
        column = lower[:, x].reshape(-1, 3)
        assert {tuple(c) for c in column} == {pc.WHITE, pc.GREY}
    assert tuple(lower[row(0.25), 30]) == pc.BLUE and tuple(lower[row(0.5), 30]) == pc.LIGHT_BLUE
    # phoneme boundary: sample 1650 -> column 16, olive from top to bottom except under the later layers
    assert pp.formant_column(1650, *SPAN, W) == 16
    assert tuple(lower[300, 16]) == pc.OLIVE and tuple(lower[row(-1.0), 16]) == pc.OLIVE and tuple(lower[300, 15]) == pc.WHITE
    assert tuple(lower[row(0.25), 16]) == pc.BLUE
    # the accuracy text at (2, 2) of the lower panel; the names under it: "aa" fits columns 0 .. 16, "h#" 16 .. 39
    acc = pc.text_mask("acc 0.7500")
    assert acc.shape[1] > W - 2 and (lower[2:9, :2] == 255).all()      # 59 columns do not fit 40: skipped, not clipped
    strip = rgb[-pc.STRIP_ROWS:]
    aa, hs = pc.text_mask("aa"), pc.text_mask("h#")
    left = 0 + (16 - 0 + 1 - aa.shape[1]) // 2
    assert np.array_equal((strip[2:9, left:left + aa.shape[1]] == 0).all(axis=2), aa)
    left = 16 + (39 - 16 + 1 - hs.shape[1]) // 2
    assert np.array_equal((strip[2:9, left:left + hs.shape[1]] == 0).all(axis=2), hs)
    assert (strip[:2] == 255).all() and (strip[9:] == 255).all()


def test_render_figure_overlays():
    k = np.arange(30)
    formant = 1500.0 + 40.0 * k                                         # 30 frames of 10 ms = 4800 samples, rising 0.25 Hz / sample
    slope = pc.FormantSlopeTrack(formant, 5, 160.0)
    assert np.allclose(np.tan(slope[1]), 0.25) and (slope[2] < 1e-6).all()
    wide = np.zeros((3, 200), np.uint8) + 9
    track = np.full((200, 5), np.nan)
    track[:, :2] = 0
    rgb = pc.RenderFigure(wide, [30, 20, 10], track, (0, 4000), RATE, formant, 10000, slope, None, 0.5, 100)
    lower = rgb[60 + pc.GAP_ROWS:60 + pc.GAP_ROWS + pc.LOWER_ROWS]
    col = pp.formant_column(10 * 160, 0, 4000, 200)                     # frame 10
    assert tuple(lower[pc.value_row(np.arctan(0.25), pc.LOWER_ROWS), col]) == pc.GREEN
    assert tuple(lower[pc.value_row(slope[2][5], pc.LOWER_ROWS), col]) == pc.RED          # p ~ 0 sits on the grey line at 0
    assert tuple(rgb[pp.formant_row(formant[10], 60, RATE, 100), col]) == pc.BLACK
    acc = pc.text_mask("acc 0.5000")
    assert np.array_equal((lower[2:9, 2:2 + acc.shape[1]] == 0).all(axis=2), acc)
    assert not (lower == np.array(pc.BLUE, np.uint8)).all(axis=2).any()   # no decisions: no curve
    none = pc.RenderFigure(wide, [30, 20, 10], track, (100, 100), RATE, formant, 10000, slope, [("aa", 0, 50)], None, 100)
    assert none.shape == rgb.shape                                        # an empty span still gives a picture


def test_parser_takes_figure_and_is_unchanged_without_it():
    a = cli.build_parser().parse_args(["cnn", "eval", "-f", "X.WAV"])
    assert "figure" not in a and "figure_width" not in a
    b = cli.build_parser().parse_args(["cnn", "evalrand", "--figure"])
    assert b.figure is True and "figure_width" not in b
    c = cli.build_parser().parse_args(["cnn", "evalnoise", "-f", "X.WAV", "-n", "3", "--figure", "--figure-width", "300", "--hop", "7"])
    assert c.figure is True and c.figure_width == 300 and c.hop == 7
    from f2cnn_amd.scripts.CNN import Evaluating
    assert Evaluating.FIGURE_WIDTH == 1600


def test_noisesweep_refuses_the_figure(capsys):
    assert cli.main(["cnn", "noisesweep", "-f", "X.WAV", "--snrs", "3", "--figure"]) == 1
    assert "not supported" in capsys.readouterr().out


def test_abi_declares_the_figure_calls():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "f2cnn_hip.h")).read(), flags=re.S)
    for name, nargs in (("f2_score_track", 11), ("f2_eval_figure_batch", 24)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    lib = ctypes.CDLL(build.build_library())
    lib.f2_version.restype = ctypes.c_int
    assert lib.f2_version() == 115      # (114 came with these two calls; 115 added f2_cnn_layers)
    assert hasattr(lib, "f2_score_track") and hasattr(lib, "f2_eval_figure_batch")
    assert callable(_lib.Context.score_track) and callable(_lib.Context.eval_figure_batch)
