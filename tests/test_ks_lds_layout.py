"""LDS layout of the 8192-point transforms of k_spectral_envelope<13, .> (f2cnn_amd/csrc/f2_fft13_merged.h, f2_fft_lds.h: Pad32,
pass0_deal): the four index maps of the 16-8-4-16 plan on 512 threads, mirrored here address by address the way the kernel forms
them (one base per thread plus compile-time offsets), under the model of the LDS the project's cost sheets use - a ds_read_b64 is
served in groups of 32 lanes, 8-byte slots mod 32; a ds_write_b64 (and each half of a ds_write2_b64) in groups of 16 contiguous
lanes, slots mod 16. No GPU needed.

Checked: every pass writes each of the 8192 points once and reads it once, at the padded address of the point (so writer and
reader agree), inside the declared array; no two lanes of a group share a slot in any of the four accesses. The layout before
(one pad per 16 points, butterflies in thread order) gives 2 lanes per slot for the last pass's reads under the same model - what
SQ_LDS_BANK_CONFLICT counted, 64 cycles per wave and row - and one pad per 32 points without the deal gives 2 for the first
pass's stores."""
import collections

import numpy as np

H, NT = 8192, 512


def pad32(i):
    return i + (i >> 5)


def pad16(i):
    return i + (i >> 4)


PAD32_SIZE = H + H // 32 + 1       # Pad32::size(H)
PAD16_SIZE = H + H // 16 + 1       # cpad_size(H)


def deal(tid):
    """pass0_deal<Pad32>: t = 64 wv + 32 (l >> 5) + 2 (l & 15) + ((l >> 4) & 1)"""
    return (tid & ~31) | ((tid & 15) << 1) | ((tid >> 4) & 1)


def deal_as_stated(tid):
    l, wv = tid & 63, tid >> 6
    return 64 * wv + 32 * (l >> 5) + 2 * (l & 15) + ((l >> 4) & 1)


# ---- the four accesses: {instruction index: [(address, point) per thread]} ----
def pass0_stores(pad, dealt):
    acc = {}
    for k in range(16):
        acc[k] = []
        for tid in range(NT):
            t = deal(tid) if dealt else tid
            acc[k].append((pad(16 * t) + k, 16 * t + k))             # dst = lds + pad(16 t); dst[k]
    return acc


def exchange_a_reads(pad, step1024):
    acc = {}
    for i in range(2):
        for j in range(8):
            acc[(i, j)] = []
            for tid in range(NT):
                l = tid & 63
                hl = l >> 5
                base8 = (l & 31) + 32 * (tid >> 6)
                b = base8 + 256 * (i + 2 * hl)
                acc[(i, j)].append((pad(b) + j * step1024, b + 1024 * j))
    return acc


def merged_stores(pad, step):
    acc = {}
    for k in range(4):
        for k2 in range(4):
            acc[(k, k2)] = []
            for tid in range(NT):
                l = tid & 63
                hl = l >> 5
                base8 = (l & 31) + 32 * (tid >> 6)
                q, plo = base8 & 15, base8 >> 4
                pos0 = q + 64 * hl + 512 * plo
                acc[(k, k2)].append((pad(pos0) + step(16 * k) + step(128 * k2), q + 16 * (k + 4 * hl) + 512 * plo + 128 * k2))
    return acc


def pass3_reads(pad, step512):
    return {j: [(pad(tid) + j * step512, tid + 512 * j) for tid in range(NT)] for j in range(16)}


def step32(s):
    return s + (s >> 5)


def step16(s):
    return s + (s >> 4)


def worst_lanes_per_slot(acc, group, slots):
    worst = 0
    for lanes in acc.values():
        for g0 in range(0, NT, group):
            count = collections.Counter(a % slots for a, _ in lanes[g0:g0 + group])
            worst = max(worst, max(count.values()))
    return worst


def check_cover(acc, pad, size):
    pts = np.array([p for lanes in acc.values() for _, p in lanes])
    adr = np.array([a for lanes in acc.values() for a, _ in lanes])
    assert len(pts) == H
    assert np.array_equal(np.sort(pts), np.arange(H))               # every point exactly once
    assert np.array_equal(adr, np.array([pad(int(p)) for p in pts]))  # at its padded address: base + immediates is exact
    assert adr.max() < size and adr.min() >= 0
    assert len(set(adr.tolist())) == H


NEW = {
    "pass-0 stores": (pass0_stores(pad32, True), 16, 16),
    "exchange-A reads": (exchange_a_reads(pad32, step32(1024)), 32, 32),
    "merged-pass stores": (merged_stores(pad32, step32), 16, 16),
    "pass-3 reads": (pass3_reads(pad32, step32(512)), 32, 32),
}
OLD = {
    "pass-0 stores": (pass0_stores(pad16, False), 16, 16),
    "exchange-A reads": (exchange_a_reads(pad16, step16(1024)), 32, 32),
    "merged-pass stores": (merged_stores(pad16, step16), 16, 16),
    "pass-3 reads": (pass3_reads(pad16, step16(512)), 32, 32),
}


def test_deal_is_a_permutation_inside_each_half_wave_and_keeps_thread_0():
    t = [deal(tid) for tid in range(NT)]
    assert t == [deal_as_stated(tid) for tid in range(NT)]
    assert t[0] == 0
    for g0 in range(0, NT, 32):
        assert sorted(t[g0:g0 + 32]) == list(range(g0, g0 + 32))
    # the sixteen lanes a store is served for hold t0 + 2 i
    for g0 in range(0, NT, 16):
        assert [x - t[g0] for x in t[g0:g0 + 16]] == list(range(0, 32, 2))


def test_every_pass_covers_the_8192_points_once_inside_the_array():
    assert PAD32_SIZE * 8 == 67592 and PAD32_SIZE < PAD16_SIZE
    for name, (acc, _, _) in NEW.items():
        check_cover(acc, pad32, PAD32_SIZE)
    for name, (acc, _, _) in OLD.items():
        check_cover(acc, pad16, PAD16_SIZE)


def test_offsets_fit_the_16_bit_field():
    # the largest compile-time offset of each access, in bytes
    assert 15 * step32(512) * 8 == 63360 < 65536
    assert 7 * step32(1024) * 8 < 65536
    assert (step32(16 * 3) + step32(128 * 3)) * 8 < 65536


def test_no_two_lanes_of_a_group_share_a_slot():
    for name, (acc, group, slots) in NEW.items():
        assert worst_lanes_per_slot(acc, group, slots) == 1, name


def test_the_model_sees_the_conflicts_the_counter_saw():
    got = {name: worst_lanes_per_slot(acc, group, slots) for name, (acc, group, slots) in OLD.items()}
    assert got["pass-3 reads"] == 2
    # (the other three accesses of the layout before are conflict-free; its exchange reads paid for the read2 forms instead)
    assert got["pass-0 stores"] == 1 and got["merged-pass stores"] == 1
    # one pad per 32 points with the butterflies in thread order: t >> 1 takes eight values in sixteen lanes
    assert worst_lanes_per_slot(pass0_stores(pad32, False), 16, 16) == 2
