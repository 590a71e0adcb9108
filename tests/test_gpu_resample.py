"""f2_resample_batch on the GPU: parity with scipy.signal.resample_poly inside the rounding bound of its dot products, exact
format conversion and mixdown, determinism, placement at odd alignments between guard bands, the argument errors, and
`cnn eval|noisesweep --resample` on a 48 kHz stereo file."""
import os

import numpy as np
import pytest
from scipy.signal import firwin, resample_poly

import speechlike
from devmem import Arena
from f2cnn_amd import _lib, cli, config, resample
from f2cnn_amd.model import F2CNNModel

pytestmark = pytest.mark.gpu

LENGTHS = (1000, 0, 1, 3, 97, 5000)
PAIRS = ((1, 3), (160, 441), (2, 1), (640, 441), (1, 6))
DTYPES = (np.uint8, np.int16, np.int32, np.float32, np.float64)


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def default_taps(up, down):
    """resample_poly's default filter for up / down, as the issue of f2_resample_batch states it"""
    half_len = 10 * max(up, down)
    return half_len, firwin(2 * half_len + 1, 1.0 / max(up, down), window=('kaiser', 5.0)) * up


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


@pytest.fixture(scope="module")
def noise_batch():
    """one ragged batch of int16 noise over the full range, and resample_poly of every utterance for every pair"""
    rng = np.random.default_rng(20240517)
    waves = [rng.integers(-32768, 32768, n).astype(np.int16) for n in LENGTHS]
    waves[0][:2] = (-32768, 32767)
    refs = {pair: [resample_poly(w.astype(np.float64), *pair) if len(w) else np.zeros(0) for w in waves] for pair in PAIRS}
    return waves, refs


def samples_of(dtype, shape, rng):
    if np.dtype(dtype).kind == "f":
        return rng.uniform(-1.0, 1.0, shape).astype(dtype)
    info = np.iinfo(dtype)
    x = rng.integers(info.min, int(info.max) + 1, shape).astype(dtype)
    x.reshape(-1)[:2] = (info.min, info.max)
    return x


def step1(x, channel):
    """include/f2cnn_hip.h, f2_resample_batch step 1 in NumPy: (frames, channels) of one of the five dtypes -> float64"""
    if x.dtype == np.uint8:
        v = (x.astype(np.float64) - 128.0) * 256.0
    elif x.dtype == np.int16:
        v = x.astype(np.float64)
    elif x.dtype == np.int32:
        v = x / 65536
    else:
        v = x.astype(np.float64) * 32768.0
    if channel >= 0:
        return v[:, channel].copy()
    s = v[:, 0].copy()
    for c in range(1, v.shape[1]):
        s = s + v[:, c]
    return s / v.shape[1]


@pytest.mark.parametrize("up,down", PAIRS)
def test_parity_with_resample_poly(ctx, noise_batch, up, down):
    waves, refs = noise_batch
    half_len, taps = default_taps(up, down)
    offsets = offsets_of([len(w) for w in waves])
    want = offsets_of([-(-len(w) * up // down) for w in waves])
    out = np.full(int(want[-1]), np.nan)
    got = ctx.resample_batch(np.concatenate(waves), _lib.PCM_I16, 1, -1, offsets, len(waves), up, down, taps, half_len, out,
                             _lib.MEM_HOST)
    np.testing.assert_array_equal(got, want)                      # the ceil rule
    # rounding bound of a dot product of T + 1 operations, once for each side, from the taps
    T = -(-(2 * half_len + 1) // up)
    padded = np.zeros(T * up)
    padded[:2 * half_len + 1] = np.abs(taps)
    l1 = padded.reshape(T, up).sum(axis=0).max()                  # max over phases p of sum_t |taps[p + t up]|
    g = (T + 1) * 2.0 ** -53 / (1.0 - (T + 1) * 2.0 ** -53)
    bound = 2.0 * g * max(float(np.abs(w.astype(np.float64)).max()) for w in waves if len(w)) * l1
    worst = 0.0
    for b, ref in enumerate(refs[(up, down)]):
        y = out[got[b]:got[b + 1]]
        assert y.shape == ref.shape
        if len(ref):
            worst = max(worst, float(np.abs(y - ref).max()))
    print(f"resample {up}/{down}: max |y - resample_poly| = {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound


@pytest.mark.parametrize("dtype", DTYPES)
def test_formats_and_channels_are_exact(ctx, dtype):
    rng = np.random.default_rng(np.dtype(dtype).itemsize * 7 + (np.dtype(dtype).kind == "f"))
    lengths = (300, 0, 1, 7)
    offsets = offsets_of(lengths)
    for channels in (1, 2, 3):
        x = samples_of(dtype, (int(offsets[-1]), channels), rng)
        for channel in sorted({-1, 0, channels - 1}):
            out = np.full(int(offsets[-1]), np.nan)
            got = ctx.resample_batch(x, resample.pcm_format(dtype), channels, channel, offsets, len(lengths), 1, 1, None, 0, out,
                                     _lib.MEM_HOST)
            np.testing.assert_array_equal(got, offsets)
            want = step1(x, channel)
            assert out.tobytes() == want.tobytes(), (dtype, channels, channel)


def test_resample_arrays_splits_the_batch(ctx, noise_batch):
    waves, refs = noise_batch
    outs = resample.resample_arrays([w for w in waves], 48000, 16000, ctx=ctx)
    assert [len(o) for o in outs] == [len(r) for r in refs[(1, 3)]]
    stereo = [np.stack([w, w], axis=1) for w in waves]
    for a, b in zip(outs, resample.resample_arrays(stereo, 48000, 16000, ctx=ctx)):
        np.testing.assert_array_equal(a, b)                       # (w + w) / 2 is w


@pytest.mark.parametrize("dtype,misalign", [(np.int16, 1), (np.uint8, 3)])
def test_determinism_and_placement(ctx, dtype, misalign):
    up, down = 160, 441
    half_len, taps = default_taps(up, down)
    rng = np.random.default_rng(99 + misalign)
    lengths = (1500, 0, 2, 701)
    offsets = offsets_of(lengths)
    x = samples_of(dtype, (int(offsets[-1]), 2), rng)
    fmt = resample.pcm_format(dtype)
    total_out = sum(_lib.resampled_length(n, up, down) for n in lengths)
    host = [np.full(total_out, np.nan) for _ in range(2)]
    for out in host:
        oo = ctx.resample_batch(x, fmt, 2, -1, offsets, len(lengths), up, down, taps, half_len, out, _lib.MEM_HOST)
    assert oo[-1] == total_out and not np.isnan(host[0]).any()
    assert host[0].tobytes() == host[1].tobytes()
    with Arena(ctx) as arena:
        arena.region("audio", dtype, x.size, misalign=misalign, role="in")      # int16 at a 2-byte offset, uint8 at an odd byte
        arena.region("out", np.float64, total_out, misalign=5, role="out")
        arena.upload("audio", x)
        od = ctx.resample_batch(arena.ptr("audio"), fmt, 2, -1, offsets, len(lengths), up, down, taps, half_len, arena.ptr("out"),
                                _lib.MEM_DEVICE)
        ctx.synchronize()
        np.testing.assert_array_equal(od, oo)
        arena.check()                                     # guards intact: nothing before out, nothing past out_offsets[B]
        assert arena.unwritten("out") == 0
        assert arena.download("out").tobytes() == host[0].tobytes()


def call(ctx, audio, fmt, channels, channel, offsets, B, up, down, taps, half_len, out, out_offsets, mem_space=_lib.MEM_HOST):
    """the C entry point itself (Context.resample_batch allocates out_offsets and refuses a NULL ctx)"""
    p = lambda a: None if a is None else a.ctypes.data
    handle = ctx.handle if ctx is not None else None
    return _lib.load().f2_resample_batch(handle, p(audio), fmt, channels, channel, p(offsets), B, up, down, p(taps), half_len,
                                         p(out), p(out_offsets), mem_space)


def test_errors(ctx):
    x = np.arange(40, dtype=np.int16)
    offsets = np.array([0, 10, 20], np.int64)
    half_len, taps = default_taps(1, 2)
    out, oo = np.zeros(64), np.zeros(3, np.int64)
    good = dict(audio=x, fmt=_lib.PCM_I16, channels=2, channel=-1, offsets=offsets, B=2, up=1, down=2, taps=taps, half_len=half_len,
                out=out, out_offsets=oo)
    assert call(ctx, **good) == _lib.F2_OK and list(oo) == [0, 5, 10]
    invalid = [dict(audio=None), dict(out=None), dict(offsets=None), dict(out_offsets=None), dict(taps=None), dict(B=-1),
               dict(channels=0), dict(channel=-2), dict(channel=2), dict(fmt=-1), dict(fmt=5), dict(up=0), dict(down=0),
               dict(half_len=-1), dict(offsets=np.array([1, 10, 20], np.int64)), dict(offsets=np.array([0, 10, 5], np.int64)),
               dict(up=2, down=4), dict(mem_space=_lib.MEM_HOST_ASYNC), dict(mem_space=7)]
    for change in invalid:
        oo[:] = -7
        assert call(ctx, **dict(good, **change)) == _lib.F2_ERR_INVALID, change
        assert (oo == -7).all(), change                             # nothing written
    assert call(None, **good) == _lib.F2_ERR_INVALID
    # identity needs no taps
    assert call(ctx, **dict(good, up=1, down=1, taps=None, half_len=0)) == _lib.F2_OK and list(oo) == [0, 10, 20]
    np.testing.assert_array_equal(out[:20], step1(x.reshape(-1, 2), -1))
    # a ratio the kernel does not cover
    big = 10 * 4099
    assert call(ctx, **dict(good, up=1, down=4099, taps=np.zeros(2 * big + 1), half_len=big)) == _lib.F2_ERR_UNSUPPORTED
    assert b"4096" in ctx.lib.f2_last_error(ctx.handle)             # the message names the limit
    assert call(ctx, **dict(good, B=0, offsets=np.zeros(1, np.int64))) == _lib.F2_OK
    assert call(ctx, **dict(good, B=0, offsets=np.zeros(1, np.int64), audio=None, out=None)) == _lib.F2_OK
    assert call(ctx, **dict(good, offsets=np.zeros(3, np.int64), audio=None, out=None)) == _lib.F2_OK and list(oo) == [0, 0, 0]


def test_commands_on_a_48_khz_stereo_file(tmp_path, monkeypatch, capsys):
    from scipy.io import wavfile
    from f2cnn_amd.scripts.CNN import Evaluating
    monkeypatch.chdir(tmp_path)
    config.write_default()
    m = F2CNNModel.glorot(7)
    m.save("last_trained_model.npz")
    n = 28800                                                      # 0.6 s at 48 kHz
    w = speechlike.make(5, n, "syllables")[0]
    stereo = np.stack([w, (w // 2).astype(np.int16)], axis=1)
    wavfile.write("rec48.WAV", 48000, stereo)
    assert cli.main(["cnn", "eval", "--file", "rec48.WAV", "--resample", "--hop", "frame", "--model", "last_trained_model.npz"]) == 0
    res = np.load("rec48.F2CNN.npz")
    rows = _lib.strided_window_count(-(-n // 3), 5, 160, 160)
    assert rows > 40 and res["labels"].shape == (rows,) and res["scores"].shape == (rows, 2)
    assert int(res["framerate"]) == 16000 and int(res["source_framerate"]) == 48000 and int(res["hop"]) == 160
    mono = resample.resample_arrays([stereo], 48000, 16000)[0]
    assert mono.shape == (-(-n // 3),)
    scores, labels = Evaluating.EvaluateOneWavArray(mono, 16000, model=m, hop=160)
    assert res["scores"].tobytes() == scores.tobytes() and res["labels"].tobytes() == labels.tobytes()
    # a file that already is 16 kHz, mono, int16: the same arrays with and without the flag
    wavfile.write("rec16.WAV", 16000, w[:9600])
    got = []
    for flag in ([], ["--resample"]):
        assert cli.main(["cnn", "eval", "--file", "rec16.WAV", "--hop", "frame", "--model", "last_trained_model.npz"] + flag) == 0
        r = np.load("rec16.F2CNN.npz")
        got.append({k: r[k] for k in ("scores", "labels", "timepoints")})
        assert ("framerate" in r.files) == bool(flag)
    for k in got[0]:
        assert got[0][k].tobytes() == got[1][k].tobytes(), k
    # the sweep at one level: its clean decisions are those of the eval run
    assert cli.main(["cnn", "noisesweep", "--file", "rec48.WAV", "--snrs", "10", "--resample", "--hop", "frame",
                     "--model", "last_trained_model.npz"]) == 0
    sweep = np.load(os.path.join("OutputWavFiles", "addedNoise", "rec48.sweep.npz"))
    assert int(sweep["framerate"]) == 16000 and int(sweep["source_framerate"]) == 48000
    np.testing.assert_array_equal(sweep["labels_clean"], res["labels"])
    assert sweep["labels_0"].shape == res["labels"].shape
    capsys.readouterr()
