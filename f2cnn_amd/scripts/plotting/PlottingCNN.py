"""Drop-in for the picture side of the reference's ``scripts/plotting/PlottingCNN.py`` (the figure ``EvaluateOneWavArray`` ends in):
where the network follows the formant and where it does not. Written from the figure's definition, without matplotlib - the
picture is an (H, W, 3) uint8 array for f2cnn_amd/png.py, W columns wide with no margins, and column x of both panels is column x
of the device's track (f2_score_track / f2_eval_figure_batch):

    upper panel   sum(ratios) rows: the `plot gtg` picture (PlottingProcessing.colour_table, rows repeated by the ERB ratios), the
                  configured formant's track in black, a red tick of TICK_ROWS rows centred on 2500 Hz in every column with a rising
                  decision and a blue one centred on 500 Hz in every column with a falling decision
                  (the reference's slice ``cnnFalling = cnnRising[start:end]`` plots the rising marks twice and never the falling
                  ones; the intent - one mark per class - is what is drawn here)
    GAP_ROWS      white rows
    lower panel   LOWER_ROWS rows spanning y in [-1.6, 1.6] as the reference's axis does (value_row), drawn in this order: white;
                  grey lines at y = 0, 0.5 and 1; an olive column at the last sample of every phoneme; a light-blue band from the
                  smallest to the largest probability of "rising" of every column that has decisions; arctan of the formant's slope
                  in green; the p-value of that slope in red; the mean probability in blue on top, consecutive non-empty columns
                  joined by a vertical run as PlottingProcessing.draw_formants joins frames. With an accuracy, ``acc 0.xxxx`` at
                  the top left.
    STRIP_ROWS    rows: every phoneme's name centred on its segment where text_mask fits between the boundaries

Legends and axis labels are not drawn.

``RenderOcclusion`` (not in the reference) is the picture of ``--occlusion``: the same upper panel over a panel of the same
geometry that shows, per channel band and time column, how far blanking the band moves the probability of "rising".
``RenderSaliency`` (not in the reference) is the picture of ``--saliency``: the same two panels, the lower one the input gradient
times the input, summed over the window's rows, per channel and time column."""
import numpy

from ..processing.FBFileReader import frame_windows
from ..processing.LabelDataGenerator import slopes_and_pvalues
from .PlottingProcessing import colour_table, draw_formants, formant_column, formant_row

TICK_ROWS, GAP_ROWS, LOWER_ROWS, STRIP_ROWS = 9, 8, 321, 12
Y_TOP, Y_SPAN = 1.6, 3.2
RISING_HZ, FALLING_HZ = 2500, 500
WHITE, BLACK = (255, 255, 255), (0, 0, 0)
RED, BLUE, GREEN = (214, 39, 40), (31, 119, 180), (44, 160, 44)
GREY, OLIVE, LIGHT_BLUE = (176, 176, 176), (110, 117, 14), (198, 219, 239)

# 5 x 7 glyphs, rows top to bottom; letters are drawn as capitals
_GLYPHS = {
    'a': ".###. #...# #...# ##### #...# #...# #...#", 'b': "####. #...# #...# ####. #...# #...# ####.",
    'c': ".###. #...# #.... #.... #.... #...# .###.", 'd': "####. #...# #...# #...# #...# #...# ####.",
    'e': "##### #.... #.... ####. #.... #.... #####", 'f': "##### #.... #.... ####. #.... #.... #....",
    'g': ".###. #...# #.... #.### #...# #...# .####", 'h': "#...# #...# #...# ##### #...# #...# #...#",
    'i': ".###. ..#.. ..#.. ..#.. ..#.. ..#.. .###.", 'j': "..### ...#. ...#. ...#. ...#. #..#. .##..",
    'k': "#...# #..#. #.#.. ##... #.#.. #..#. #...#", 'l': "#.... #.... #.... #.... #.... #.... #####",
    'm': "#...# ##.## #.#.# #.#.# #...# #...# #...#", 'n': "#...# ##..# #.#.# #..## #...# #...# #...#",
    'o': ".###. #...# #...# #...# #...# #...# .###.", 'p': "####. #...# #...# ####. #.... #.... #....",
    'q': ".###. #...# #...# #...# #.#.# #..#. .##.#", 'r': "####. #...# #...# ####. #.#.. #..#. #...#",
    's': ".#### #.... #.... .###. ....# ....# ####.", 't': "##### ..#.. ..#.. ..#.. ..#.. ..#.. ..#..",
    'u': "#...# #...# #...# #...# #...# #...# .###.", 'v': "#...# #...# #...# #...# #...# .#.#. ..#..",
    'w': "#...# #...# #...# #.#.# #.#.# ##.## #...#", 'x': "#...# #...# .#.#. ..#.. .#.#. #...# #...#",
    'y': "#...# #...# .#.#. ..#.. ..#.. ..#.. ..#..", 'z': "##### ....# ...#. ..#.. .#... #.... #####",
    '0': ".###. #...# #..## #.#.# ##..# #...# .###.", '1': "..#.. .##.. ..#.. ..#.. ..#.. ..#.. .###.",
    '2': ".###. #...# ....# ...#. ..#.. .#... #####", '3': "##### ...#. ..#.. ...#. ....# #...# .###.",
    '4': "...#. ..##. .#.#. #..#. ##### ...#. ...#.", '5': "##### #.... ####. ....# ....# #...# .###.",
    '6': "..##. .#... #.... ####. #...# #...# .###.", '7': "##### ....# ...#. ..#.. .#... .#... .#...",
    '8': ".###. #...# #...# .###. #...# #...# .###.", '9': ".###. #...# #...# .#### ....# ...#. .##..",
    '#': ".#.#. .#.#. ##### .#.#. ##### .#.#. .#.#.", '-': "..... ..... ..... ##### ..... ..... .....",
    '.': "..... ..... ..... ..... ..... .##.. .##..", ':': "..... .##.. .##.. ..... .##.. .##.. .....",
    '%': "##..# ##..# ...#. ..#.. .#... #..## #..##", ' ': "..... ..... ..... ..... ..... ..... .....",
}
GLYPHS = {ch: numpy.array([[c == '#' for c in row] for row in rows.split()], dtype=bool) for ch, rows in _GLYPHS.items()}


def value_row(y, height):
    """Row of the value y in a panel of `height` rows that spans y = 1.6 (row 0) .. -1.6 (the last row)."""
    return int(numpy.rint((height - 1) * (Y_TOP - y) / Y_SPAN))


def text_mask(string):
    """(7, 6 * len - 1) bool: the string in the 5 x 7 glyphs, one empty column between characters. Knows a-z (capitals are
    folded), 0-9, # - . : % and the space; anything else raises KeyError."""
    string = string.lower()
    mask = numpy.zeros((7, max(6 * len(string) - 1, 0)), dtype=bool)
    for i, ch in enumerate(string):
        mask[:, 6 * i:6 * i + 5] = GLYPHS[ch]
    return mask


def FormantSlopeTrack(track_hz, radius, samples_per_frame):
    """(sample positions, arctan(slope), p) for every frame k in radius .. len - radius - 1 of a formant track (Hz, one value per
    frame): the least-squares slope of the 2 * radius + 1 frames around k against their sample positions j * samples_per_frame -
    Hz per sample, as in the reference - and the p-value of pearsonr(frames, fitted line); frame k stands at sample
    k * samples_per_frame."""
    track = numpy.asarray(track_hz, dtype=numpy.float64)
    k = numpy.arange(radius, len(track) - radius)
    positions = k * float(samples_per_frame)
    if not len(k):
        return positions, numpy.zeros(0), numpy.zeros(0)
    # frame_windows truncates t / samples_per_frame (asked at the middle of frame k, clear of rounding) and, like the reference,
    # refuses a window that ends with the track's last frame: one more frame stands behind it, in no window
    windows = frame_windows(numpy.append(track, track[-1]), (k + 0.5) * float(samples_per_frame), radius, samples_per_frame)
    slope, p = slopes_and_pvalues(windows, positions, float(samples_per_frame))
    return positions, numpy.arctan(slope), p


def _draw_curve(panel, columns, rows, colour):
    """points (column, row) in order, consecutive ones joined by a vertical run in the later point's column; a point outside the
    panel (row None included) is skipped and breaks the join"""
    height, width = panel.shape[:2]
    previous = None
    for col, row in zip(columns, rows):
        if row is None or not (0 <= col < width and 0 <= row < height):
            previous = None
            continue
        top, bottom = (min(previous, row), max(previous, row)) if previous is not None else (row, row)
        panel[top:bottom + 1, col] = colour
        previous = row


def _rows_of(values, height):
    return [value_row(v, height) if numpy.isfinite(v) else None for v in values]


def _put_text(panel, mask, top, left, colour):
    """the mask at (top, left) if it lies inside the panel; returns whether it was drawn"""
    h, w = mask.shape
    if top < 0 or left < 0 or top + h > panel.shape[0] or left + w > panel.shape[1]:
        return False
    panel[top:top + h, left:left + w][mask] = colour
    return True


def RenderFigure(levels, ratios, track, span, framerate, formant_hz=None, sampPeriod=10000, slope_track=None, phonemes=None,
                 accuracy=None, low_freq=100):
    """The figure as (sum(ratios) + GAP_ROWS + LOWER_ROWS + STRIP_ROWS, W, 3) uint8 (layout: the module's docstring).
    levels (C, W) uint8 and track (W, 5) float64 {rows, rising, mean, min, max} come from f2_eval_figure_batch for the samples
    span = (start, end) of a file at `framerate`; formant_hz: the formant's track (one value per frame of sampPeriod microseconds)
    or None; slope_track: FormantSlopeTrack's triple or None; phonemes: [(name, first sample, last sample)] or None; accuracy: a
    number or None."""
    levels, track = numpy.asarray(levels), numpy.asarray(track, dtype=numpy.float64)
    width = levels.shape[1]
    start, end = int(span[0]), int(span[1])
    upper = colour_table()[numpy.repeat(levels, ratios, axis=0)]
    h1 = upper.shape[0]
    if formant_hz is not None:
        draw_formants(upper, [formant_hz], sampPeriod, framerate, start, end, low_freq)
    rising, falling = track[:, 1] > 0, track[:, 0] - track[:, 1] > 0
    for hz, columns, colour in ((RISING_HZ, rising, RED), (FALLING_HZ, falling, BLUE)):
        centre = formant_row(hz, h1, framerate, low_freq)
        upper[max(centre - TICK_ROWS // 2, 0):max(centre + TICK_ROWS // 2 + 1, 0), columns] = colour

    lower = numpy.full((LOWER_ROWS, width, 3), 255, numpy.uint8)
    for y in (0.0, 0.5, 1.0):
        lower[value_row(y, LOWER_ROWS)] = GREY
    column_of = (lambda sample: formant_column(sample, start, end, width)) if end > start else (lambda sample: -1)
    for _, _, last in phonemes or ():
        if 0 <= column_of(last) < width:
            lower[:, column_of(last)] = OLIVE
    filled = track[:, 0] > 0
    for x in numpy.flatnonzero(filled & numpy.isfinite(track[:, 3]) & numpy.isfinite(track[:, 4])):
        top, bottom = value_row(track[x, 4], LOWER_ROWS), value_row(track[x, 3], LOWER_ROWS)
        lower[max(top, 0):max(bottom + 1, 0), x] = LIGHT_BLUE
    if slope_track is not None:
        positions, angle, p = slope_track
        columns = [column_of(t) for t in positions]
        _draw_curve(lower, columns, _rows_of(angle, LOWER_ROWS), GREEN)
        _draw_curve(lower, columns, _rows_of(p, LOWER_ROWS), RED)
    _draw_curve(lower, range(width), [r if f else None for r, f in zip(_rows_of(track[:, 2], LOWER_ROWS), filled)], BLUE)
    if accuracy is not None:
        _put_text(lower, text_mask("acc {:.4f}".format(float(accuracy))), 2, 2, BLACK)

    strip = numpy.full((STRIP_ROWS, width, 3), 255, numpy.uint8)
    for name, first, last in phonemes or ():
        try:
            mask = text_mask(name)
        except KeyError:
            continue
        c0, c1 = column_of(first), column_of(last)
        left = c0 + (c1 - c0 + 1 - mask.shape[1]) // 2
        if left > c0 and left + mask.shape[1] <= c1:          # between the boundaries, touching neither
            _put_text(strip, mask, 2, left, BLACK)
    gap = numpy.full((GAP_ROWS, width, 3), 255, numpy.uint8)
    return numpy.concatenate([upper, gap, lower, strip], axis=0)


def diverging_colours(values, scale):
    """(..., 3) uint8 for values in [-scale, scale]: BLUE at -scale, white at 0, RED at +scale, linear in between (a ramp
    symmetric about 0); scale <= 0 or a value that is not finite: white / GREY."""
    values = numpy.asarray(values, dtype=numpy.float64)
    finite = numpy.isfinite(values)
    t = numpy.clip(numpy.where(finite, values, 0.0) / scale, -1.0, 1.0) if scale > 0 else numpy.zeros(values.shape)
    end = numpy.where((t >= 0)[..., None], numpy.array(RED, numpy.float64), numpy.array(BLUE, numpy.float64))
    rgb = numpy.rint(255.0 + numpy.abs(t)[..., None] * (end - 255.0)).astype(numpy.uint8)
    rgb[~finite] = GREY
    return rgb


def RenderOcclusion(levels, ratios, map, patches, span, framerate, formant=None, sampPeriod=10000, low_freq=100):
    """The occlusion figure as (2 * sum(ratios) + GAP_ROWS, W, 3) uint8, column x of both panels column x of the device's map
    (f2_occlusion_map / f2_eval_occlusion_batch):

        upper panel   the gammatonegram as RenderFigure draws it, the formant's track in black
        GAP_ROWS      white rows
        lower panel   the same geometry: channel c takes the ERB row height ratios[c] and, in column x, the colour of mean d =
                      map[k][x][2] of the patch k that blanks it (the mean over the patches that do, where bands overlap) on
                      diverging_colours, scaled to the largest |mean d| of the file: red where blanking the band raises P(rising),
                      blue where it lowers it, white where it changes nothing. A column without rows is grey; a channel no patch
                      blanks is white. The formant's track in black again.

    levels (C, W) uint8; map (K, W, 4) float64 {rows, flips, mean d, mean |d|}; patches (K, 4) {r0, r1, c0, c1}, every one spanning
    all rows of the window (the picture has one value per channel and column); span = (start, end) samples of a file at
    `framerate`; formant: its track in Hz, one value per frame of sampPeriod microseconds, or None."""
    levels, map = numpy.asarray(levels), numpy.asarray(map, dtype=numpy.float64)
    patches = numpy.asarray(patches).reshape(-1, 4)
    channels, width = levels.shape
    start, end = int(span[0]), int(span[1])
    upper = colour_table()[numpy.repeat(levels, ratios, axis=0)]
    total, count = numpy.zeros((channels, width)), numpy.zeros((channels, 1))
    for k, (_, _, c0, c1) in enumerate(patches):
        total[c0:c1] += map[k, :, 2]
        count[c0:c1] += 1
    with numpy.errstate(invalid='ignore', divide='ignore'):
        mean_d = numpy.where(count > 0, total / count, 0.0)
    mean_d[:, map[0, :, 0] == 0] = numpy.nan           # (the columns own the same rows whatever the patch)
    finite = numpy.abs(map[..., 2][numpy.isfinite(map[..., 2])])
    lower = numpy.repeat(diverging_colours(mean_d, finite.max() if finite.size else 0.0), ratios, axis=0)
    if formant is not None:
        for panel in (upper, lower):
            draw_formants(panel, [formant], sampPeriod, framerate, start, end, low_freq)
    gap = numpy.full((GAP_ROWS, width, 3), 255, numpy.uint8)
    return numpy.concatenate([upper, gap, lower], axis=0)


def RenderSaliency(levels, ratios, map, span, framerate, formant=None, sampPeriod=10000, low_freq=100):
    """The saliency figure as (2 * sum(ratios) + GAP_ROWS, W, 3) uint8, column x of both panels column x of the device's map
    (f2_saliency_map / f2_eval_saliency_batch):

        upper panel   the gammatonegram as RenderFigure draws it, the formant's track in black
        GAP_ROWS      white rows
        lower panel   the same geometry: channel c takes the ERB row height ratios[c] and, in column x, the colour of the mean of
                      sum_r G x = map[c][x][1] on diverging_colours, scaled to the largest magnitude of the file: red where the
                      channel's energy pushes P(rising) up, blue where it pushes it down, white where it does nothing. A column
                      without rows is grey. The formant's track in black again.

    levels (C, W) uint8; map (C, W, 3) float64 {rows, mean G x, mean |G|}; span = (start, end) samples of a file at `framerate`;
    formant: its track in Hz, one value per frame of sampPeriod microseconds, or None."""
    levels, map = numpy.asarray(levels), numpy.asarray(map, dtype=numpy.float64)
    width = levels.shape[1]
    start, end = int(span[0]), int(span[1])
    upper = colour_table()[numpy.repeat(levels, ratios, axis=0)]
    gx = numpy.where(map[..., 0] > 0, map[..., 1], numpy.nan)
    finite = numpy.abs(gx[numpy.isfinite(gx)])
    lower = numpy.repeat(diverging_colours(gx, finite.max() if finite.size else 0.0), ratios, axis=0)
    if formant is not None:
        for panel in (upper, lower):
            draw_formants(panel, [formant], sampPeriod, framerate, start, end, low_freq)
    gap = numpy.full((GAP_ROWS, width, 3), 255, numpy.uint8)
    return numpy.concatenate([upper, gap, lower], axis=0)
