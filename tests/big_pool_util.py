"""KV pools larger than 4 GiB for test_gpu_big_pool.py: every pool of that module is a typed view of ONE uint8 storage
of NBYTES, and a case uses only slots of a "high window" -- slots whose offset from the pool's base is at least 2^32
elements, chosen so that every 32-bit truncation a kernel could make of that offset (of the element offset, of the byte
offset, of the partial products page * page_stride or slot * tok_stride, signed or unsigned) lands at a small offset
INSIDE the storage.  A kernel that truncates then reads sentinel bytes or writes over a canary: it fails a comparison,
it never leaves the allocation.

The arithmetic here is plain Python integers (test_big_pool_util.py holds it to a brute-force restatement on the CPU);
the torch helpers at the end only cut views."""
from collections import namedtuple

TWO31, TWO32 = 1 << 31, 1 << 32
WINDOW_BYTES = 32 << 20             # no window (and no page rounding in front of it) is larger than this
V_OFFSET = WINDOW_BYTES             # the V view's base lies one window above the K view's: their windows are disjoint
MID_BASE = TWO32                    # base of the views that use offsets in [2^31, 2^32): "below the view" is storage
NBYTES = 2 * TWO32 + 4 * WINDOW_BYTES
WINDOW_SLOTS = 1024
SCALE_BASES = (TWO31, TWO31 + (1 << 30))   # the K / V scale-byte views of a 4-bit pool: far from every window and alias
SCALE_GUARD_ROWS = 16
SENTINEL = 0xFF                     # bf16 / f16 0xFFFF and e4m3fn 0xFF are NaNs; 4-bit data 0xFF is (-6, -6)

# name -> (kv heads, row width in elements per head, bytes per element, page size, layout); "hnd" = [pages, H, page, D]
# pages, "nhd" = [slots, H, D] rows (page_size only groups them).  4-bit data rows are D / 2 BYTES per head.
GEOMETRIES = {
    "bf16_h8_d128": (8, 128, 2, 1, "nhd"),
    "bf16_h8_d128_hnd": (8, 128, 2, 16, "hnd"),
    "bf16_h2_d128": (2, 128, 2, 1, "nhd"),
    "bf16_h2_d128_hnd": (2, 128, 2, 16, "hnd"),
    "bf16_h2_d64": (2, 64, 2, 1, "nhd"),
    "bf16_h2_d64_hnd": (2, 64, 2, 16, "hnd"),
    "bf16_h2_d80": (2, 80, 2, 1, "nhd"),
    "bf16_h2_d96": (2, 96, 2, 1, "nhd"),
    "bf16_h2_d256_hnd": (2, 256, 2, 16, "hnd"),
    "bf16_mla": (1, 576, 2, 1, "nhd"),
    "fp8_h2_d128": (2, 128, 1, 1, "nhd"),
    "fp8_h2_d128_hnd": (2, 128, 1, 16, "hnd"),
    "fp8_mla": (1, 576, 1, 1, "nhd"),
    "mx4_h2_d128": (2, 64, 1, 16, "nhd"),
    "mx4_mla": (1, 288, 1, 16, "nhd"),
}

Window = namedtuple("Window", "lo hi page_size row_bytes byte_lo byte_hi alias alias_slots")
# lo, hi: the slot range.  byte_lo, byte_hi: its bytes relative to the view's base.  alias: [(rel_lo, rel_hi)] byte
# ranges relative to the view's base (negative = below the view) that the truncations hit.  alias_slots: the slots of
# the view (>= 0) whose rows intersect those ranges.


def _wrap(x, signed):
    x %= TWO32
    return x - TWO32 if signed and x >= TWO31 else x


def high_window(row_elems, elem_bytes, page_size=1, layout="nhd", n_slots=WINDOW_SLOTS, start=None, span=None):
    """The window of a pool whose slot holds `row_elems` elements of `elem_bytes` bytes (all kv heads), in pages of
    `page_size` slots.  start / span (elements): offsets used lie in [start, start + span); by default [2^32, 2^32 +
    2^30), or [2^32, 2^32 + 2^31) for byte-addressed pools.  The window starts on a page, so that page * page_stride
    itself lies in the range; the layout only names how a page's elements are ordered, which the window (whole
    pages) does not depend on."""
    assert layout in ("nhd", "hnd")
    if start is None:
        start, span = TWO32, (TWO31 if elem_bytes == 1 else 1 << 30)
    page_stride = row_elems * page_size
    first = -(-start // page_stride)
    pages = -(-n_slots // page_size)
    e_lo, e_hi = first * page_stride, (first + pages) * page_stride
    assert e_hi <= start + span and (e_hi - e_lo) * elem_bytes <= WINDOW_BYTES and e_lo * elem_bytes - start * elem_bytes <= WINDOW_BYTES
    b_lo, b_hi = e_lo * elem_bytes, e_hi * elem_bytes
    alias = set()
    for signed in (False, True):
        # the element offset kept in 32 bits, then scaled; the byte offset kept in 32 bits.  Over the window each is the
        # true offset minus a constant (checked): the partial products page * page_stride / slot * tok_stride are the
        # offsets of page / row starts, and what is added to them afterwards is smaller than a page
        for lo, hi in ((_wrap(e_lo, signed) * elem_bytes, _wrap(e_hi - 1, signed) * elem_bytes + elem_bytes),
                       (_wrap(b_lo, signed), _wrap(b_hi - 1, signed) + 1)):
            assert hi - lo == b_hi - b_lo, "a 32-bit wrap inside the window"
            if lo != b_lo:
                alias.add((lo, hi))
    alias = sorted(alias)
    row_bytes = row_elems * elem_bytes
    slots = set()
    for lo, hi in alias:
        for p in range(max(lo, 0) // (row_bytes * page_size), -(-max(hi, 0) // (row_bytes * page_size))):
            slots.update(range(p * page_size, (p + 1) * page_size))
    return Window(first * page_size, (first + pages) * page_size, page_size, row_bytes, b_lo, b_hi, alias, frozenset(slots))


def mid_window(row_elems, elem_bytes, page_size=1, layout="nhd", n_slots=WINDOW_SLOTS):
    """Offsets in [2^31, 2^31 + 2^20) elements: a signed 32-bit element offset goes BELOW the view, so the view must
    sit at storage byte MID_BASE."""
    return high_window(row_elems, elem_bytes, page_size, layout, n_slots, start=TWO31, span=1 << 20)


def geometry_window(name, **kw):
    h, d, es, page, layout = GEOMETRIES[name]
    return high_window(h * d, es, page, layout, **kw)


# ---- torch helpers ---------------------------------------------------------------------------------------------------
def pool_view(storage, base, dtype, name, win):
    """The pool of geometry `name` as a view of `storage` that starts at byte `base` and ends with the window."""
    h, d, es, page, layout = GEOMETRIES[name]
    assert dtype.itemsize == es and base % 16 == 0 and base + win.byte_hi <= storage.numel()
    flat = storage[base: base + win.byte_hi].view(dtype)
    return flat.view(win.hi // page, h, page, d) if layout == "hnd" else flat.view(win.hi, h, d)


def window_rows(pool, win):
    """The window's part of a pool view (pages of an HND pool)."""
    return pool[win.lo // win.page_size: win.hi // win.page_size] if pool.dim() == 4 else pool[win.lo: win.hi]


def fill_alias(storage, base, win):
    for lo, hi in win.alias:
        storage[base + lo: base + hi] = SENTINEL


def alias_intact(storage, base, win):
    return all(bool((storage[base + lo: base + hi] == SENTINEL).all()) for lo, hi in win.alias)


def scale_ranges(which, scale_row_bytes, win):
    """Storage byte ranges of a 4-bit pool's scale view [slots, scale_row_bytes] (`which`: 0 = K, 1 = V): (view, window,
    [guards]).  Scale bytes sit 8x lower than the data (offsets near 2^29: no 32-bit truncation moves them), so
    their canaries are the guard rows on both sides of the window."""
    base = SCALE_BASES[which]
    lo, hi = base + win.lo * scale_row_bytes, base + win.hi * scale_row_bytes
    g = SCALE_GUARD_ROWS * scale_row_bytes
    return (base, hi), (lo, hi), [(lo - g, lo), (hi, hi + g)]


def scale_view(storage, which, scale_row_bytes, win):
    (lo, hi), _, _ = scale_ranges(which, scale_row_bytes, win)
    return storage[lo:hi].view(win.hi, scale_row_bytes)
