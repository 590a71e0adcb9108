"""The bookkeeping of tests/devmem.py on a NumPy backing store: placement, poison, and what check() reports."""
import numpy as np
import pytest

from devmem import Arena, ArenaViolation, BOUNDARY, GUARD, NumpyStore, poison

DTYPES = [np.float64, np.float32, np.int16, np.uint8, np.int32, np.int64]
# (dtype, misalign): the odd placements of the device test, the last slot of a 128-byte line included
PLACEMENTS = [(np.float64, 0), (np.float64, 1), (np.float64, 5), (np.float64, 15), (np.float32, 1), (np.float32, 3),
              (np.float32, 31), (np.int16, 1), (np.int16, 3), (np.uint8, 1), (np.uint8, 3), (np.int32, 1), (np.int64, 1)]


def laid_out(count=37):
    """one region per placement, roles in turn; the `in` / `inout` ones uploaded"""
    a = Arena(make_store=NumpyStore)
    roles = {}
    for i, (dt, k) in enumerate(PLACEMENTS):
        name = f"r{i}"
        roles[name] = ("in", "out", "inout")[i % 3]
        a.region(name, dt, count + i, misalign=k, role=roles[name])
    for i, (dt, k) in enumerate(PLACEMENTS):
        if roles[f"r{i}"] != "out":
            a.upload(f"r{i}", np.arange(count + i).astype(dt))
    return a, roles


def test_requested_misalignments_are_honoured_for_every_dtype():
    a, _ = laid_out()
    assert a.store.base % BOUNDARY == 0
    ends = []
    for i, (dt, k) in enumerate(PLACEMENTS):
        r = a._regions[f"r{i}"]
        assert a.ptr(f"r{i}") == a.store.base + r.start
        assert a.ptr(f"r{i}") % BOUNDARY == k * np.dtype(dt).itemsize
        assert a.ptr(f"r{i}") % np.dtype(dt).itemsize == 0                   # natural alignment always
        assert r.start - r.slot >= GUARD and r.slot_end - r.end >= GUARD      # a full guard band on both sides
        assert r.slot % BOUNDARY == 0
        ends.append((r.slot, r.slot_end))
    assert all(e0[1] == e1[0] for e0, e1 in zip(ends, ends[1:]))             # one allocation, slot after slot
    assert ends[-1][1] == a._size == len(a.store.mem)


@pytest.mark.parametrize("dt", DTYPES)
def test_poison_per_dtype(dt):
    a = Arena(make_store=NumpyStore)
    a.region("x", dt, 10, misalign=1, role="out")
    a.region("y", dt, 4, misalign=3 if np.dtype(dt).itemsize < 8 else 5, role="in")
    r = a._regions["x"]
    a.ptr("x")
    whole = a.store.mem[r.slot:r.slot_end].view(dt)
    if np.dtype(dt).kind == "f":
        assert np.isnan(whole).all()
        assert len(set(whole.view(f"u{np.dtype(dt).itemsize}").tolist())) == 1   # one payload
    elif np.dtype(dt) == np.int16:
        assert set(whole.tolist()) == {32767, -32768} and (whole[1:] != whole[:-1]).all()
    else:
        assert (whole == whole[0]).all() and whole[0] != 0
    assert a.unwritten("x") == 10                                            # an out region starts as poison ...
    got = a.download("x")
    got[3] = 1
    a.store.write(r.start, got.view(np.uint8))
    assert a.unwritten("x") == 9                                             # ... and a written element no longer is
    np.testing.assert_array_equal(poison(dt, 4, 2).view(np.uint8), poison(dt, 6)[2:].view(np.uint8))


def test_upload_download_roundtrip_and_untouched_check():
    a, roles = laid_out()
    a.check()
    for i, (dt, k) in enumerate(PLACEMENTS):
        if roles[f"r{i}"] != "out":
            np.testing.assert_array_equal(a.download(f"r{i}"), np.arange(37 + i).astype(dt))
    a.check()
    with pytest.raises(ValueError):
        a.upload("r0", np.zeros(3))
    with pytest.raises(RuntimeError):
        a.region("late", np.float32, 1)


@pytest.mark.parametrize("name", ["r0", "r1", "r3", "r5", "r8", "r12"])
@pytest.mark.parametrize("where", ["just_before", "just_after", "far_lead", "far_tail"])
def test_one_changed_guard_byte_is_named_with_its_distance(name, where):
    a, _ = laid_out()
    r = a._regions[name]
    at, kind, dist = {"just_before": (r.start - 1, "before", -1), "just_after": (r.end, "after", 0),
                      "far_lead": (r.slot, "before", r.slot - r.start),
                      "far_tail": (r.slot_end - 1, "after", r.slot_end - 1 - r.end)}[where]
    a.store.mem[at] ^= 0x40
    with pytest.raises(ArenaViolation) as e:
        a.check()
    assert (e.value.region, e.value.where, e.value.distance, e.value.changed) == (name, kind, dist, 1)
    assert name in str(e.value) and f"{dist:+d} bytes" in str(e.value)
    a.store.mem[at] ^= 0x40
    a.check()


def test_a_changed_byte_inside_an_in_region_fails_and_inside_an_out_region_does_not():
    a, roles = laid_out()
    for name, role in roles.items():
        r = a._regions[name]
        a.store.mem[r.start + 5] ^= 0x01
        if role == "in":
            with pytest.raises(ArenaViolation) as e:
                a.check()
            assert (e.value.region, e.value.where, e.value.distance) == (name, "inside", 5)
            a.store.mem[r.start + 5] ^= 0x01
        else:
            a.check()                                                        # out / inout: the call may write it


def test_the_lowest_changed_address_is_reported():
    a, _ = laid_out()
    r3, r7 = a._regions["r3"], a._regions["r7"]
    a.store.mem[r7.start - 9] = 0
    a.store.mem[r3.end + 16] = 0
    with pytest.raises(ArenaViolation) as e:
        a.check()
    assert (e.value.region, e.value.where, e.value.distance, e.value.changed) == ("r3", "after", 16, 2)


def test_empty_regions_and_bad_requests():
    a = Arena(make_store=NumpyStore)
    a.region("none", np.float32, 0, misalign=3, role="out")
    a.region("some", np.uint8, 5, misalign=1, role="in")
    assert a.ptr("none") % BOUNDARY == 12 and a.download("none").size == 0 and a.unwritten("none") == 0
    a.check()
    b = Arena(make_store=NumpyStore)
    for bad in (dict(dtype=np.float16, count=1), dict(dtype=np.float32, count=-1), dict(dtype=np.float64, count=1, misalign=32),
                dict(dtype=np.float32, count=1, role="scratch")):
        with pytest.raises(ValueError):
            b.region("x", **bad)
    with pytest.raises(ValueError):
        Arena()
