"""A device arena for placement tests: named regions inside ONE allocation, each at a chosen element misalignment past a
256-byte boundary and fenced by guard bands on both sides, so that a kernel's stray write shows up as a changed guard byte and a
stray read returns poison (tests/test_gpu_device_placement.py; the bookkeeping alone: tests/test_devmem_layout.py).

    arena = Arena(ctx)                                   # or Arena(make_store=NumpyStore): a NumPy array stands in for the device
    arena.region("wave", np.int16, n, misalign=1, role="in")
    arena.region("gfb", np.float64, C * n, misalign=15, role="out")
    arena.upload("wave", wave)
    ctx.erb_filterbank_batch(arena.ptr("wave"), ..., arena.ptr("gfb"), _lib.MEM_DEVICE)
    ctx.synchronize()
    arena.check()                                        # guards and `in` regions byte for byte as they were
    assert arena.unwritten("gfb") == 0                   # no element of the output still holds its pre-fill
    gfb = arena.download("gfb")

Layout of one region's slot (slots follow each other, every slot starts on a 256-byte boundary):

    | lead guard: GUARD + misalign * itemsize bytes | region: count * itemsize bytes | tail guard: >= GUARD bytes, to a boundary |

GUARD is 64 KiB: wider than any tile, line or pair a kernel stores and wider than a whole float64 row of the short test cases, so
"one row too far" still lands inside the allocation, in a guard. The whole slot is filled with the poison of the region's dtype on
the region's own element grid: a NaN with a recognisable payload for the float types, alternating 32767 / -32768 for int16, a
fixed non-zero pattern for the other integers. `out` regions keep that fill until the call under test writes them.
"""
import numpy as np

GUARD = 64 * 1024
BOUNDARY = 256

# (bit pattern as an unsigned integer of the element's width) per dtype; int16 alternates between two
_POISON = {
    np.dtype(np.float64): (0x7FF8DEAD0000BEEF,),
    np.dtype(np.float32): (0x7FDEAD01,),
    np.dtype(np.int16): (0x7FFF, 0x8000),
    np.dtype(np.uint8): (0xA5,),
    np.dtype(np.int32): (0x5A5AA5A5,),
    np.dtype(np.int64): (0x5A5AA5A55A5AA5A5,),
}
_ROLES = ("in", "out", "inout")


def poison(dtype, count, first=0):
    """`count` poison elements of `dtype` as they stand at element indices first, first + 1, ... of a slot"""
    dtype = np.dtype(dtype)
    pat = _POISON[dtype]
    u = np.dtype(f"u{dtype.itemsize}")
    idx = (first + np.arange(count)) % len(pat)
    return np.array(pat, dtype=u)[idx].view(dtype)


class ArenaViolation(AssertionError):
    """check() found a changed byte: `region` is the region it belongs to or adjoins, `where` is "before" (lead guard; `distance`
    is negative, -1 = the byte just in front of the region), "after" (tail guard; 0 = the byte just past the region's end) or
    "inside" (an `in` region; distance from its first byte)."""

    def __init__(self, region, where, distance, changed):
        self.region, self.where, self.distance, self.changed = region, where, int(distance), int(changed)
        edge = {"before": "start", "after": "end", "inside": "start"}[where]
        super().__init__(f"region '{region}': first changed byte {self.distance:+d} bytes from its {edge} ({where}); "
                         f"{changed} bytes of the arena changed that the call must not write")


class NumpyStore:
    """Host stand-in for a device allocation: the same read / write / base / free as DeviceStore"""

    def __init__(self, nbytes):
        raw = np.zeros(nbytes + BOUNDARY, np.uint8)
        skip = -raw.ctypes.data % BOUNDARY
        self.mem = raw[skip:skip + nbytes]
        self.base = self.mem.ctypes.data

    def read(self, offset, nbytes):
        return self.mem[offset:offset + nbytes].copy()

    def write(self, offset, data):
        self.mem[offset:offset + len(data)] = data

    def free(self):
        self.mem = None


class DeviceStore:
    """One device allocation of an f2cnn_amd._lib.Context"""

    def __init__(self, ctx, nbytes):
        self.ctx, self.base = ctx, ctx.malloc(nbytes)

    def read(self, offset, nbytes):
        out = np.empty(nbytes, np.uint8)
        if nbytes:
            self.ctx.synchronize()
            self.ctx.d2h(out, self.base + offset)
        return out

    def write(self, offset, data):
        if len(data):
            self.ctx.h2d(self.base + offset, np.ascontiguousarray(data))
            self.ctx.synchronize()

    def free(self):
        if self.base:
            self.ctx.synchronize()
            self.ctx.free(self.base)
            self.base = 0


class _Region:
    def __init__(self, name, dtype, count, misalign, role, slot):
        self.name, self.dtype, self.count, self.misalign, self.role = name, np.dtype(dtype), int(count), int(misalign), role
        self.slot = slot                                             # first byte of the lead guard
        self.start = slot + GUARD + self.misalign * self.dtype.itemsize
        self.end = self.start + self.count * self.dtype.itemsize
        self.slot_end = -(-self.end // BOUNDARY) * BOUNDARY + GUARD  # one past the tail guard

    @property
    def nbytes(self):
        return self.end - self.start


class Arena:
    def __init__(self, ctx=None, make_store=None):
        if (ctx is None) == (make_store is None):
            raise ValueError("give a context or a store factory")
        self._make = make_store if make_store is not None else (lambda nbytes: DeviceStore(ctx, nbytes))
        self._regions = {}
        self._size = 0
        self.store = None
        self._image = None            # what the arena must hold outside `out` / `inout` regions

    # ---- layout (before the first transfer) ----
    def region(self, name, dtype, count, misalign=0, role="in"):
        dtype = np.dtype(dtype)
        if self.store is not None:
            raise RuntimeError("the arena is laid out: declare every region before the first ptr / upload / download / check")
        if name in self._regions:
            raise ValueError(f"region '{name}' exists")
        if dtype not in _POISON:
            raise ValueError(f"no poison for {dtype}")
        if role not in _ROLES:
            raise ValueError(f"role must be one of {_ROLES}")
        if count < 0 or misalign < 0 or misalign * dtype.itemsize >= BOUNDARY:
            raise ValueError("count >= 0 and 0 <= misalign * itemsize < 256")
        r = _Region(name, dtype, count, misalign, role, self._size)
        self._regions[name] = r
        self._size = r.slot_end
        return r

    def _commit(self):
        if self.store is not None:
            return
        if not self._regions:
            raise RuntimeError("no regions")
        self.store = self._make(self._size)
        if self.store.base % BOUNDARY:
            raise RuntimeError("the allocation does not start on a 256-byte boundary")
        image = np.empty(self._size, np.uint8)
        for r in self._regions.values():
            n = (r.slot_end - r.slot) // r.dtype.itemsize
            image[r.slot:r.slot_end] = poison(r.dtype, n).view(np.uint8)
        self._image = image
        self.store.write(0, image)

    # ---- use ----
    def ptr(self, name):
        self._commit()
        return self.store.base + self._regions[name].start

    def upload(self, name, array):
        self._commit()
        r = self._regions[name]
        a = np.ascontiguousarray(array, dtype=r.dtype).reshape(-1)
        if a.size != r.count:
            raise ValueError(f"region '{name}' holds {r.count} elements, not {a.size}")
        b = a.view(np.uint8)
        self._image[r.start:r.end] = b
        self.store.write(r.start, b)

    def download(self, name):
        self._commit()
        r = self._regions[name]
        return self.store.read(r.start, r.nbytes).view(r.dtype)

    def unwritten(self, name):
        """elements of the region that hold the bit pattern it was pre-filled with"""
        r = self._regions[name]
        u = np.dtype(f"u{r.dtype.itemsize}")
        first = (r.start - r.slot) // r.dtype.itemsize
        return int((self.download(name).view(u) == poison(r.dtype, r.count, first).view(u)).sum())

    def check(self):
        """Every guard band and every `in` region byte for byte as laid out / uploaded, else ArenaViolation for the changed
        byte at the lowest address."""
        self._commit()
        now = self.store.read(0, self._size)
        watched = np.ones(self._size, bool)
        for r in self._regions.values():
            if r.role != "in":
                watched[r.start:r.end] = False
        bad = np.flatnonzero((now != self._image) & watched)
        if not len(bad):
            return
        at = int(bad[0])
        for r in self._regions.values():
            if r.slot <= at < r.slot_end:
                if at < r.start:
                    raise ArenaViolation(r.name, "before", at - r.start, len(bad))
                if at >= r.end:
                    raise ArenaViolation(r.name, "after", at - r.end, len(bad))
                raise ArenaViolation(r.name, "inside", at - r.start, len(bad))
        raise RuntimeError("changed byte outside every slot")

    def free(self):
        if self.store is not None:
            self.store.free()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False
