"""A call's outputs are a function of its arguments, never of the calls that came before it on the same f2_ctx.

Every entry point runs on a long-lived context that remembers things between calls: the offsets and the coefficient table it last
uploaded (and what hangs off the table: eligibility for the spectral route, the padding that route needs), the routing lists, six
slots of spectral tables, the low-pass power table, pair lists and hand-off offsets, the time-split filterbank's transition table
and its unit queue, the resampling table, twiddle tables, the networks' scale sets, grow-only scratch shared by some 45 entry
points, the pinned upload ring with its side buffers, and the sticky error words. tests/call_history.py holds the catalogue of
calls and the runner; every test here is ONE sequence on ONE context, named after the state it attacks, of the form A, B, A where
B differs from A in exactly the way the cache key must notice. After every call: raw-byte equality with that call's fresh result
(its result on a context of its own, which the first test holds against the entry point's independent reference).

Entry points of the catalogue: erb_filterbank_batch (plain, k1_split forced, k1_queue = 1, general table, a second channel group,
float64 samples), envelope_batch (every size class, float and float64 FFT, env_pair 0 / 1), filterbank_envelope_fused (both routes,
int16 and float64 waves, with and without gfb), gather_windows, input_batch, cnn_forward, eval_batch_strided, lowpass_levels,
reverb_levels, channel_mix_levels, resample_batch, eval_cutoff_sweep, gammatonegram_batch."""
import numpy as np
import pytest

import call_history as ch
from call_history import F32, fused
from f2cnn_amd import _lib

pytestmark = pytest.mark.gpu

CATALOGUE = ch.catalogue()


@pytest.fixture
def ctx():
    with ch.context() as c:
        yield c


# ---- the catalogue: fresh results against the independent references ------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CATALOGUE))
def test_fresh_result_against_the_entry_points_own_reference(name):
    ch.fresh(CATALOGUE[name])


def test_the_runner_accepts_a_repeated_call_and_reports_a_changed_byte(ctx):
    """the runner itself: a call repeated on one context is its fresh result, and a changed byte is reported"""
    call = CATALOGUE[next(iter(CATALOGUE))]
    ch.replay(ctx, [call, call])
    got = dict(call.run(ctx))
    got["gfb"] = bytes([got["gfb"][0] ^ 1]) + got["gfb"][1:]
    assert ch.differences(call, got, ch.fresh(call)) == [f"'gfb': 1 of {len(got['gfb']) // 8} elements differ, the first at element 0"]


# ---- offsets cache (f2_upload_offsets) ---------------------------------------------------------------------------------------------------
def _split(flat, at):
    return (ch.frozen(flat[:at]), ch.frozen(flat[at:]))


def test_offsets_with_the_same_count_and_total_but_another_split(ctx):
    """[0, 5000, 9000] against [0, 4000, 9000] over the same 9000 samples, then the first offsets with another wave"""
    flat, other = ch.wave(7100, 9000), ch.wave(7101, 9000)
    a = fused((), waves=_split(flat, 5000), tag="9000 samples split at 5000")
    b = fused((), waves=_split(flat, 4000), tag="9000 samples split at 4000")
    a2 = fused((), waves=_split(other, 5000), tag="9000 other samples split at 5000")
    ch.replay(ctx, [a, b, a, a2, a, b])
    two = [fused((), waves=w, tag=t, route="two_kernel") for w, t in ((_split(flat, 5000), "9000 samples split at 5000"),
                                                                      (_split(flat, 4000), "9000 samples split at 4000"))]
    ch.replay(ctx, [two[0], two[1], two[0], a, two[1]])


def test_offsets_through_the_entry_points_that_share_the_cache(ctx):
    """fused, reverb_levels, lowpass_levels: the two offset arrays alternate between the entry points that all upload through
    f2_upload_offsets"""
    flat = ch.wave(7100, 9000)
    fa = fused((), waves=_split(flat, 5000), tag="9000 samples split at 5000")
    fb = fused((), waves=_split(flat, 4000), tag="9000 samples split at 4000")
    ra, rb = ch.reverb_levels((5000, 4000), taps=(3, 40)), ch.reverb_levels((4000, 5000), taps=(3, 40))
    la, lb = ch.lowpass_levels((5000, 4000), C=5, cutoffs=(50.0,)), ch.lowpass_levels((4000, 5000), C=5, cutoffs=(50.0,))
    ch.replay(ctx, [fa, rb, la, fb, ra, lb, fa, lb, rb, fa])


# ---- coefficient cache and what hangs off it (f2_upload_coefs, spec_coefs_ok, spec_min_pad) -------------------------------------------
ROW = 8064        # 128 padding samples in the 8192-sample class: enough for the bank from 1000 Hz (64), not for the one from 100 Hz (256)


def test_coefficient_tables_of_one_size(ctx):
    """Same C, tables that differ by the lowest frequency (100 Hz / 1000 Hz: routed 0 / 1 for a row with 128 padding samples), by
    eligibility (the general table is never routed) and in one channel's row"""
    low, high = fused((ROW,), tab="erb100", routed=0), fused((ROW,), tab="erb1000", routed=1)
    general, row = fused((ROW,), tab="general", routed=0), fused((ROW,), tab="erb1000_row", routed=1)
    ch.replay(ctx, [low, high, general, low, high, row, high, general, row, low])


def test_coefficient_tables_through_the_filterbank_and_the_two_kernel_route(ctx):
    tabs = ("erb100", "erb1000", "general", "erb100", "erb1000_row", "erb1000")
    ch.replay(ctx, [ch.filterbank((1599, 33, 4099), tab=t) for t in tabs])
    ch.replay(ctx, [fused((ROW, 300), tab=t, route="two_kernel") for t in tabs])


def test_coefficient_tables_of_another_channel_count(ctx):
    five, eight = fused((ROW, 4097), C=5, tab="erb1000", routed=2), fused((ROW, 4097), C=8, tab="erb1000", routed=2)
    ch.replay(ctx, [five, eight, five, ch.filterbank((1599, 33), C=8), ch.filterbank((1599, 33), C=5), eight, five])


# ---- spectral table slots: six (table, length class) pairs, the oldest out ----------------------------------------------------------------
CLASSES = (4097, 8193, 16385, 32769)          # the shortest row of each length class of the spectral kernels
BANKS = ("erb100", "erb1000")


def test_spectral_table_slots_are_built_evicted_and_rebuilt(ctx):
    """Two banks x four length classes = eight pairs for six slots: each pair twice round, so every one is built, evicted and built
    again. Then, with the slots full of the last six pairs, ONE call whose batch holds all four classes of the bank visited first:
    its first two classes evict that bank's own last two, which the same call needs two launches later - evictions between the
    launches of one call. The batch also holds a row with a click 5 samples before its end, which the accuracy guard sends back:
    the two-kernel fallback runs in the same call."""
    pairs = [fused((n,), tab=t, routed=1) for t in BANKS for n in CLASSES]
    waves = tuple(ch.wave(7300 + i, n) for i, n in enumerate(CLASSES)) + (ch.late_click(16000),)
    all_classes = fused((), waves=waves, tab=BANKS[0], tag="every class and a late click", routed=5, flagged=1)
    ch.replay(ctx, pairs + pairs + [all_classes, pairs[-1], all_classes] + pairs[:3])


# ---- low-pass power table (spec_lptab, keyed on a1 alone) ---------------------------------------------------------------------------------
def test_lowpass_table_follows_the_cutoff(ctx):
    """50 -> 5 -> 50 -> off -> 50 -> 49.999 -> 50 Hz on the spectral route"""
    at = {c: fused((4097,), cutoff=c, routed=1) for c in (50.0, 5.0, 49.999)}
    off = fused((4097,), lpf=False, routed=1)
    ch.replay(ctx, [at[50.0], at[5.0], at[50.0], off, at[50.0], at[49.999], at[50.0]])


def test_lowpass_table_serves_every_workgroup_size(ctx):
    """One cutoff across rows of 4097, 8193, 16385 and 32769 samples (256 / 512 / 1024 threads and the long-row kernel), in
    separate calls both ways round and in one call: the table is keyed on the filter coefficient alone (lowpass_table,
    f2_spectral.hip), its per-thread entries do not depend on the workgroup size"""
    one = [fused((n,), routed=1) for n in CLASSES]
    together = fused(CLASSES, routed=4)
    ch.replay(ctx, one + one[::-1] + [together, one[0], together, fused((4097,), cutoff=5.0, routed=1), together])


# ---- routing lists (spec_meta_host) --------------------------------------------------------------------------------------------------------
def test_routing_lists_that_hold_the_same_words(ctx):
    """(5000, 9000) and (5000, 6000) both concatenate to [0, 0 | 0, 1]: one list per class against one list of two; then the same
    routed set in a batch of three; then a batch routed, not routed (spectral = 0) and routed again"""
    a, b = fused((5000, 9000), routed=2), fused((5000, 6000), routed=2)
    three = fused((5000, 9000, 300), routed=2)
    plain = fused((5000, 9000), route="two_kernel", routed=0)
    ch.replay(ctx, [a, b, a, three, a, plain, a, b, plain, b])


# ---- pair lists and hand-off offsets (pair_list_host, handoff_off_host) -------------------------------------------------------------------
@pytest.mark.parametrize("env_pair", [1, 0])
def test_pair_lists_and_handoff_offsets(ctx, env_pair):
    """Rows of 32769..65536 samples on the two-kernel route, on-chip (env_pair = 1) and four-step: the long rows change places in
    the batch, and a 70000-sample row joins them"""
    orders = [(40000, 300, 40000), (300, 40000, 40000), (40000, 300, 40000, 70000), (70000, 300, 40000, 40000)]
    calls = [fused(lens, C=4, route="two_kernel", env_pair=env_pair) for lens in orders]
    ch.replay(ctx, [calls[0], calls[1], calls[0], calls[2], calls[0], calls[3], calls[2], calls[1]])


def test_pair_lists_between_env_pair_settings(ctx):
    a = {p: fused((40000, 300, 40000), C=4, route="two_kernel", env_pair=p) for p in (0, 1)}
    b = {p: fused((300, 40000, 40000), C=4, route="two_kernel", env_pair=p) for p in (0, 1)}
    ch.replay(ctx, [a[1], b[0], a[1], a[0], b[1], a[0], ch.envelope((32769,), env_pair=1), a[1], ch.envelope((32769,), env_pair=0), b[1]])


# ---- time-split filterbank table and queue (k1_mtab, k1_order) ---------------------------------------------------------------------------
def test_time_split_table_follows_the_segment_length_and_the_coefficients(ctx):
    """B = 1 rows of 16000, 8000 and 16000 samples under the library's own policy (another segment length L), the same L with another
    table, and forced segment counts"""
    n16, n8 = ch.filterbank((16000,), mode="auto"), ch.filterbank((8000,), mode="auto")
    other = ch.filterbank((16000,), mode="auto", tab="erb1000")
    forced = ch.filterbank((1599, 33, 4099), mode="split")
    ch.replay(ctx, [n16, n8, n16, other, n16, forced, n8, other, forced, n16])


def test_unit_queue_back_to_back(ctx):
    """k1_queue = 1 on two ragged batches with equal unit counts and different length orders, in device memory so that nothing
    waits between them: the order list and its queue counter are rewritten while the previous launch may still run"""
    a, b = ch.filterbank((3000, 40, 1500, 700), mode="queue"), ch.filterbank((40, 700, 3000, 1500), mode="queue")
    two_groups = ch.filterbank((1599, 300), C=65, mode="queue")
    ch.replay_enqueued([(ctx, c) for c in (a, b, a, b, two_groups, a, two_groups, b)])


# ---- resample table (rs_tab) --------------------------------------------------------------------------------------------------------------
def test_resample_table_follows_ratio_and_taps(ctx):
    """(160, 441) with the default taps, the same ratio and length with taps of another Kaiser beta, (1, 3), and back"""
    default, other, third = ch.resample(160, 441, 5.0), ch.resample(160, 441, 8.0), ch.resample(1, 3, 5.0)
    ch.replay(ctx, [default, other, default, third, default, other, third, other])


# ---- scratch growth and shrink -------------------------------------------------------------------------------------------------------------
def _scratch_round():
    first = ch.eval_batch_strided()
    return [first, ch.gammatonegram(), ch.eval_cutoff_sweep(), ch.reverb_levels(), first, ch.fused((16385, 32769), C=4),
            ch.eval_cutoff_sweep(), ch.lowpass_levels(), ch.gammatonegram(), ch.channel_mix_levels(), first]


def test_scratch_small_large_small_in_host_memory(ctx):
    """Entry points that share stage_in / stage_out / stage_aux, levels, meta, xbuf, dense_in, gather_log: small, large, small"""
    ch.replay(ctx, _scratch_round())


def test_scratch_small_large_small_with_caller_device_buffers(ctx):
    """the same round with every buffer in the caller's device memory, between guard bands checked after each call"""
    ch.replay_in_arenas(ctx, _scratch_round())


# ---- upload ring and side buffers (f2_upload_async) ----------------------------------------------------------------------------------------
# The constants of f2_upload_async (f2_api.hip): RING = 8 MiB of pinned memory; an upload above RING / 4 = 2 MiB = 2 097 152 bytes
# goes through one of at most four side buffers instead. `centers` of f2_gather_windows is 8 bytes per window and always a host
# array, so 240 000 windows are 1 920 000 bytes (the largest round count under the limit: four such uploads fill 7.68 MB of the
# ring, the fifth wraps round onto the first) and 300 000 windows are 2 400 000 bytes (above it: calls five and six find all four
# side buffers in use). Should the constants move, move the counts with them.
UP_RING, UP_LIMIT, UP_SIDE_BUFFERS = 8 << 20, (8 << 20) // 4, 4
UP_N, UP_C, UP_RADIUS, UP_STEP = 4000, 2, 1, 1


@pytest.mark.parametrize("windows", [240_000, 300_000], ids=["ring", "side_buffers"])
def test_uploads_pending_in_the_ring_and_in_the_side_buffers(ctx, windows):
    """Six calls back to back in device memory, each with its own centres and its own output buffer, one wait at the end: every
    output is env[:, centres + step (k - radius)] cast to float32, bit for bit"""
    nbytes, calls = 8 * windows, 6
    if windows == 240_000:
        assert nbytes <= UP_LIMIT < 8 * (windows + 25_000) and (calls - 1) * nbytes > UP_RING
    else:
        assert nbytes > UP_LIMIT and calls > UP_SIDE_BUFFERS
    rng = np.random.default_rng(windows)
    env = rng.random((UP_C, UP_N)) * 40 + 1e-3
    rows = 2 * UP_RADIUS + 1
    out_bytes = 4 * windows * rows * UP_C
    centres = [rng.permutation(UP_RADIUS * UP_STEP + np.arange(windows) % (UP_N - 2 * UP_RADIUS * UP_STEP)).astype(np.int64)
               for _ in range(calls)]
    d_env, d_out = ctx.malloc(env.nbytes), [ctx.malloc(out_bytes) for _ in range(calls)]
    try:
        with ch.stop_on_gpu_fault():
            ctx.h2d(d_env, env)
            for d in d_out:
                ctx.memset(d, ch.FILL, out_bytes)
            ctx.synchronize()
            for cs, d in zip(centres, d_out):
                ctx.gather_windows(d_env, UP_C, UP_N, cs, windows, UP_RADIUS, UP_STEP, False, d, _lib.MEM_DEVICE)
            ctx.synchronize()
            for i, (cs, d) in enumerate(zip(centres, d_out)):
                got = np.empty((windows, rows, UP_C), np.float32)
                ctx.d2h(got, d)
                want = env[:, cs[:, None] + UP_STEP * (np.arange(rows) - UP_RADIUS)[None, :]].transpose(1, 2, 0).astype(np.float32)
                assert got.tobytes() == np.ascontiguousarray(want).tobytes(), f"call {i} of {calls}"
    finally:
        for d in [d_env] + d_out:
            ctx.free(d)


# ---- failed calls leave nothing behind -------------------------------------------------------------------------------------------------------
def _refused(ctx):
    """F2_ERR_INVALID: a wave type that does not exist (tests/test_gpu_filterbank.py::test_bad_arguments)"""
    with pytest.raises(_lib.F2Error) as e:
        ctx.erb_filterbank_batch(np.zeros(4, np.int16), 7, np.array([0, 4], np.int64), np.zeros((4, 10)), 1, 4, np.zeros(16), ch.HOST)
    assert e.value.code == _lib.F2_ERR_INVALID


def _unsupported(ctx):
    """F2_ERR_UNSUPPORTED: a resampling ratio beyond the kernel's reach (tests/test_gpu_resample.py::test_errors)"""
    big = 10 * 4099
    with pytest.raises(_lib.F2Error) as e:
        ctx.resample_batch(np.arange(40, dtype=np.int16), _lib.PCM_I16, 2, -1, np.array([0, 10, 20], np.int64), 2, 1, 4099,
                           np.zeros(2 * big + 1), big, np.zeros(64), ch.HOST)
    assert e.value.code == _lib.F2_ERR_UNSUPPORTED


def _nonpositive(ctx):
    """F2_ERR_NONPOSITIVE, raised after the kernels ran: the second utterance is silent, so its envelope rows are zero and their
    windows cannot be normalised"""
    lens = (2500, 2500)
    flat = np.concatenate([ch.wave(7400, lens[0]), np.zeros(lens[1], np.int16)])
    n = sum(_lib.strided_window_count(m, ch.RADIUS, ch.STEP, 160) for m in lens)
    scores, labels = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
    with pytest.raises(_lib.F2Error) as e:
        ctx.eval_batch_strided(ch.network_on(ctx, ch.R, ch.EVAL_C), flat, _lib.WAVE_I16, ch.offsets_of(lens), ch.table("erb100", ch.EVAL_C),
                               2, ch.EVAL_C, True, 50.0, F32, ch.RADIUS, ch.STEP, 160, scores, labels, ch.HOST)
    assert e.value.code == _lib.F2_ERR_NONPOSITIVE


@pytest.mark.parametrize("profiling", [False, True], ids=["plain", "profiling_on_around_the_failure"])
def test_failed_calls_leave_nothing_behind(ctx, profiling):
    """A refused call, an unsupported one and one that fails after its kernels ran, each between two calls of the catalogue: the
    next call returns F2_OK (ch.replay's calls raise otherwise) and its fresh bits. With profiling switched on around the failing
    call, whose event pool the upload ring shares"""
    around = [fused((4097, 300, 8193)), ch.resample(), ch.eval_batch_strided(), ch.eval_cutoff_sweep(), ch.gather_windows()]
    for i, fail in enumerate((_refused, _unsupported, _nonpositive, _refused, _nonpositive)):
        ch.replay(ctx, [around[i], around[(i + 1) % len(around)]])
        if profiling:
            ctx.prof_enable(True)
        try:
            fail(ctx)
        finally:
            if profiling:
                ctx.prof_enable(False)
        ch.replay(ctx, [around[(i + 2) % len(around)], around[i]])


# ---- two networks on one context -------------------------------------------------------------------------------------------------------------
def test_two_networks_and_two_input_bounds_on_one_context(ctx):
    """Handles for an 11 x 128 and a 13 x 40 network alternate; then inputs in [0, 1), in [0, 1024) and in [0, 1) again on the same
    handle (one set of scales per input bound)"""
    wide, tall = ch.cnn_forward(11, 128), ch.cnn_forward(13, 40)
    wide_big, tall_big = ch.cnn_forward(11, 128, scale=1024.0), ch.cnn_forward(13, 40, scale=1024.0)
    ch.replay(ctx, [wide, tall, wide, tall, wide, wide_big, wide, tall_big, tall, wide_big, tall_big, wide])


# ---- two contexts on one device --------------------------------------------------------------------------------------------------------------
def test_two_contexts_alternate_on_one_device(ctx):
    """As the file drivers use pipeline_contexts(2): context A runs the spectral route while context B runs the two-kernel route on
    another batch, device pointers, eight alternations with changing shapes, nothing waits until all sixteen calls are enqueued"""
    spectral = [fused((4097, 9000)), fused((8193,)), fused((16385, 5000)), fused((ROW,), tab="erb1000")]
    two_kernel = [fused((300, 2000), C=4, route="two_kernel"), fused((40000, 300, 40000), C=4, route="two_kernel"),
                  fused((5000,), C=4, route="two_kernel"), fused((300, 40000, 40000), C=4, route="two_kernel")]
    with ch.context() as other:
        pairs = []
        for i in range(8):
            pairs += [(ctx, spectral[(3 * i) % 4]), (other, two_kernel[(3 * i + 1) % 4])]
        ch.replay_enqueued(pairs)


# ---- a seeded shuffle: the net under the targeted sequences ----------------------------------------------------------------------------------
def test_forty_calls_in_a_seeded_order(ctx):
    names = list(CATALOGUE)
    order = [names[i] for i in np.random.default_rng(0).integers(0, len(names), 40)]
    try:
        ch.replay(ctx, [CATALOGUE[n] for n in order])
    except AssertionError:
        print("order of the shuffle:\n  " + "\n  ".join(order))
        raise
