"""f2cnn_amd/noise.py, the filters of `cnn noisesweep --colours`: every filter handed out has sum h^2 = 1 and, where it is designed,
symmetric taps of odd length; the designed shapes follow their stated magnitudes; LikeFIR follows the spectrum of a recording within
the Welch estimate's own scatter; and what cannot be a filter is refused with ValueError. No GPU."""
import numpy as np
import pytest
from scipy.io import wavfile

from f2cnn_amd import noise

RATE = 16000


def response_db(h, freqs, rate=RATE):
    """20 log10 |H(f)| of the taps h at the frequencies freqs, by the definition of the transform"""
    n = np.arange(len(h))
    return 20 * np.log10(np.abs(np.exp(-2j * np.pi * np.outer(freqs, n) / rate) @ h))


def check_invariants(h, symmetric=True):
    assert h.dtype == np.float64 and h.ndim == 1 and h.flags["C_CONTIGUOUS"] and np.isfinite(h).all()
    assert abs(np.dot(h, h) - 1) <= 1e-12
    assert len(h) <= noise.MAX_TAPS
    if symmetric:
        assert len(h) % 2 == 1 and np.array_equal(h, h[::-1])


def pink_recording(n=32000, seed=2024):
    """a seeded white sequence through ColourFIR('pink'), the filter's transient cut off"""
    h = noise.ColourFIR("pink", RATE)
    return np.convolve(np.random.default_rng(seed).standard_normal(n + len(h) - 1), h, "valid")


def write_wav(path, x, rate=RATE):
    wavfile.write(str(path), rate, (np.asarray(x) / np.abs(x).max() * 30000).astype(np.int16))
    return str(path)


# ---- the invariants of everything handed out ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", noise.COLOURS)
@pytest.mark.parametrize("taps,rate", [(1025, 16000), (129, 16000), (2047, 16000), (3, 8000), (1025, 44100)])
def test_colour_filters_are_normalised_symmetric_and_odd(name, taps, rate):
    h = noise.ColourFIR(name, rate, taps)
    check_invariants(h)
    assert len(h) == (1 if name == "white" else taps)


def test_white_is_one_tap_of_exactly_one():
    for taps in (1, 5, 1025):
        h = noise.ColourFIR("white", RATE, taps)
        assert h.tolist() == [1.0] and h.dtype == np.float64
    assert noise.ColourFIR("pink", RATE, 1).tolist() == [1.0]
    assert noise.MAX_TAPS == 2048


def test_like_and_load_results_keep_the_invariants(tmp_path):
    path = write_wav(tmp_path / "pink.wav", pink_recording(8000))
    for taps in (1025, 65):
        h = noise.LikeFIR(path, RATE, taps)
        check_invariants(h)
        assert len(h) == taps
    sym = np.array([0.25, -1.0, 3.0, -1.0, 0.25])
    np.save(tmp_path / "sym.npy", sym)
    h = noise.LoadFIR(str(tmp_path / "sym.npy"))
    check_invariants(h)
    assert np.allclose(h, sym / np.sqrt(np.dot(sym, sym)), rtol=1e-15)
    np.save(tmp_path / "any.npy", np.array([1, -2, 0, 4], np.int32))             # integers, even length, not symmetric: taken as they are
    h = noise.LoadFIR(str(tmp_path / "any.npy"))
    check_invariants(h, symmetric=False)
    assert np.allclose(h, np.array([1, -2, 0, 4]) / np.sqrt(21.0), rtol=1e-15)
    np.save(tmp_path / "long.npy", np.ones(noise.MAX_TAPS, np.float32))           # the longest filter the library takes
    check_invariants(noise.LoadFIR(str(tmp_path / "long.npy")), symmetric=False)


# ---- the shapes ---------------------------------------------------------------------------------------------------------------
SHAPE_FREQS = np.array([62.5, 125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0, 7000.0])


def stated_db(name, freqs):
    """the magnitudes of the option's documentation, written out again: dB relative to 500 Hz"""
    f = np.asarray(freqs, dtype=np.float64)
    if name == "pink":
        mag = np.maximum(f, 20.0) ** -0.5
    elif name == "brown":
        mag = 1.0 / np.maximum(f, 20.0)
    else:
        mag = np.where(f < 100, (f / 100) ** 2, np.where(f <= 500, 1.0, (f / 500) ** -1.5))
    ref = {"pink": 500.0 ** -0.5, "brown": 1 / 500.0, "speech": 1.0}[name]
    return 20 * np.log10(mag / ref)


@pytest.mark.parametrize("name", ["pink", "brown", "speech"])
def test_designed_filters_follow_their_stated_magnitude(name):
    """Within 0.5 dB at 1025 taps and 16 kHz. The recipe (8192-point grid, irfft, Hann window), prototyped on its own before the
    module was written, deviates by at most 0.10 dB (pink), 0.27 dB (brown), 0.38 dB (speech; at 62.5 Hz and at the corners):
    0.5 dB is that figure with a small margin, not a figure taken from this code."""
    h = noise.ColourFIR(name, RATE, 1025)
    got = response_db(h, SHAPE_FREQS)
    got -= got[3]
    dev = got - stated_db(name, SHAPE_FREQS)
    print(name, "deviation in dB at", SHAPE_FREQS.tolist(), np.round(dev, 3).tolist())
    assert np.abs(dev).max() <= 0.5
    assert np.array_equal(noise.Magnitude(name, SHAPE_FREQS) > 0, np.ones(8, bool))
    assert np.allclose(20 * np.log10(noise.Magnitude(name, SHAPE_FREQS) / noise.Magnitude(name, [500.0])), stated_db(name, SHAPE_FREQS),
                       atol=1e-9)


def test_speech_shape_falls_nine_db_per_octave_above_500_hz():
    h = noise.ColourFIR("speech", RATE, 1025)
    got = response_db(h, np.array([1000.0, 2000.0, 4000.0]))
    assert np.allclose(np.diff(got), -20 * np.log10(2 ** 1.5), atol=0.05)         # -9.03 dB
    assert "convention" in noise.ColourFIR.__doc__ and "not a fit" in noise.ColourFIR.__doc__


# ---- LikeFIR ------------------------------------------------------------------------------------------------------------------
LIKE_FREQS = np.arange(250.0, 4000.5, 125.0)       # every eighth bin of the 1024-sample frames, 250 Hz to 4 kHz
# The Welch estimate's own scatter on this kind of input, measured with NumPy alone (numpy_welch_db below; 300 seeded white
# sequences of 32 000 samples through the pink filter, 61 Hann frames of 1024 with 512 overlap each): the standard deviation of a
# bin's level in dB about the pink line, the mean offset over LIKE_FREQS removed, is 0.564 dB (0.52 to 0.62 over the frequencies).
WELCH_SCATTER_DB = 0.564
LIKE_TOLERANCE_DB = 4 * WELCH_SCATTER_DB           # 2.26 dB


def numpy_welch_db(x):
    """level in dB of the Welch estimate at LIKE_FREQS about the pink line, its mean removed: NumPy alone"""
    frames = np.lib.stride_tricks.sliding_window_view(x, 1024)[::512]
    power = (np.abs(np.fft.rfft(frames * np.hanning(1024), axis=1)) ** 2).mean(axis=0)
    dev = 10 * np.log10(power[(LIKE_FREQS / (RATE / 1024)).astype(int)]) - stated_db("pink", LIKE_FREQS)
    return dev - dev.mean()


def test_the_stated_welch_scatter_is_what_numpy_measures():
    dev = np.array([numpy_welch_db(pink_recording(seed=s)) for s in range(60)])
    print("scatter of the Welch estimate in dB", dev.std())
    assert abs(dev.std() / WELCH_SCATTER_DB - 1) < 0.1


def test_like_fir_follows_the_spectrum_of_a_pink_recording(tmp_path):
    x = pink_recording()
    assert len(x) == 32000
    h = noise.LikeFIR(write_wav(tmp_path / "pink.wav", x), RATE)
    assert len(h) == 1025
    dev = response_db(h, LIKE_FREQS) - stated_db("pink", LIKE_FREQS)
    dev -= dev.mean()
    print("LikeFIR about the pink line in dB: max", np.abs(dev).max(), "std", dev.std(), "tolerance", LIKE_TOLERANCE_DB)
    assert np.abs(dev).max() <= LIKE_TOLERANCE_DB
    # and it tells colours apart: the same test against the brown line fails by far
    other = response_db(h, LIKE_FREQS) - stated_db("brown", LIKE_FREQS)
    assert np.abs(other - other.mean()).max() > 2 * LIKE_TOLERANCE_DB


def test_welch_magnitude_is_the_mean_over_hann_frames():
    x = pink_recording(4000, seed=5)
    frames = np.lib.stride_tricks.sliding_window_view(x, 1024)[::512]
    want = np.sqrt((np.abs(np.fft.rfft(frames * np.hanning(1024), axis=1)) ** 2).mean(axis=0))
    assert len(frames) == 6 and np.allclose(noise.WelchMagnitude(x), want, rtol=1e-12)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taps", [0, -3, 4, 1024, 2.5, 2049, 4097])
def test_bad_tap_counts_are_refused(taps, tmp_path):
    with pytest.raises(ValueError, match="2048" if taps in (2049, 4097) else "odd"):
        noise.ColourFIR("pink", RATE, taps)
    path = write_wav(tmp_path / "pink.wav", pink_recording(4000))
    with pytest.raises(ValueError):
        noise.LikeFIR(path, RATE, taps)


def test_unknown_colours_and_rates_are_refused():
    with pytest.raises(ValueError, match="purple"):
        noise.ColourFIR("purple", RATE)
    for rate in (0, -1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="framerate"):
            noise.ColourFIR("pink", rate)


def test_like_fir_refusals(tmp_path):
    x = pink_recording(4000)
    path = write_wav(tmp_path / "pink.wav", x)
    with pytest.raises(ValueError, match="8000"):                                # worded like LoadRIR's
        noise.LikeFIR(path, 8000)
    try:
        noise.LikeFIR(path, 8000)
    except ValueError as e:
        assert "pink.wav" in str(e) and "16000 Hz" in str(e) and "resample it first" in str(e)
    stereo = str(tmp_path / "stereo.wav")
    wavfile.write(stereo, RATE, np.stack([x, x], axis=1).astype(np.int16))
    with pytest.raises(ValueError, match="stereo.wav.*2 channels"):
        noise.LikeFIR(stereo, RATE)
    silent = str(tmp_path / "silent.wav")
    wavfile.write(silent, RATE, np.zeros(4000, np.int16))
    with pytest.raises(ValueError, match="silent.wav"):
        noise.LikeFIR(silent, RATE)
    short = write_wav(tmp_path / "short.wav", x[:1023])
    with pytest.raises(ValueError, match="short.wav.*1023"):
        noise.LikeFIR(short, RATE)
    assert len(noise.LikeFIR(write_wav(tmp_path / "frame.wav", x[:1024]), RATE)) == 1025   # a single frame is enough


@pytest.mark.parametrize("name,array,word", [
    ("empty", np.zeros(0), "empty.npy"), ("nan", np.array([1.0, np.nan]), "nan.npy"), ("inf", np.array([np.inf, 1.0]), "inf.npy"),
    ("zero", np.zeros(5), "zero.npy"), ("long", np.ones(2049), r"2049 taps \(at most 2048\)"), ("matrix", np.ones((3, 3)), "matrix.npy"),
    ("complex", np.ones(3, np.complex128), "complex.npy")])
def test_load_fir_refusals(tmp_path, name, array, word):
    path = str(tmp_path / (name + ".npy"))
    np.save(path, array)
    with pytest.raises(ValueError, match=word):
        noise.LoadFIR(path)


def test_specs():
    assert noise.SpecName("pink") == "pink" and noise.SpecName("like:/a/b/babble.wav") == "babble" and noise.SpecName("fir:taps.npy") == "taps"
    assert np.array_equal(noise.FromSpec("speech", RATE, 65), noise.ColourFIR("speech", RATE, 65))
