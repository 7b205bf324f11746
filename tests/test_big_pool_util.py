"""big_pool_util (the windows of test_gpu_big_pool.py) on the CPU, by brute-force integer arithmetic over every slot,
head and row end of every geometry the module uses: the offsets are where the module says, every 32-bit truncation of
them stays inside the storage, and the alias ranges hold every such truncation and none of the window."""
import pytest

import big_pool_util as bp

BASES = (0, bp.V_OFFSET)


def _element_offsets(name, slot):
    """(true element offset, the partial product a kernel forms first, what it adds afterwards) for the first and last
    element of every head's row of `slot`, as include/radix_hip.h states the addressing."""
    h, d, es, page, layout = bp.GEOMETRIES[name]
    if layout == "hnd":
        page_stride, tok_stride, head_stride = h * page * d, d, page * d
    else:
        page_stride, tok_stride, head_stride = page * h * d, h * d, d
    out = []
    for head in range(h):
        for col in (0, d - 1):
            rest = (slot % page) * tok_stride + head * head_stride + col
            out.append(((slot // page) * page_stride + rest, (slot // page) * page_stride, rest))
            if layout == "nhd":  # linear pools multiply the slot itself
                out.append((slot * tok_stride + head * head_stride + col, slot * tok_stride, head * head_stride + col))
    return out


def _truncations(off, part, rest, es):
    """byte offsets (relative to the view) of every way to lose the upper half: the element offset or the byte offset
    in 32 bits, the partial product in elements or in bytes in 32 bits -- each unsigned and signed"""
    out = set()
    for signed in (False, True):
        wrap = lambda x: bp._wrap(x, signed)  # noqa: E731
        out |= {wrap(off) * es, wrap(off * es), (wrap(part) + rest) * es, wrap(part * es) + rest * es}
    return out


def _check(name, win, base, start, span):
    h, d, es, page, layout = bp.GEOMETRIES[name]
    assert win.lo % page == 0 and win.hi % page == 0 and win.hi - win.lo >= bp.WINDOW_SLOTS
    assert base + win.byte_hi <= bp.NBYTES
    ranges = [(base + lo, base + hi) for lo, hi in win.alias]
    assert ranges, "no truncation moves the window: it tests nothing"
    for lo, hi in ranges:  # inside the storage, and not the window itself
        assert 0 <= lo < hi <= bp.NBYTES
        assert hi <= base + win.byte_lo or lo >= base + win.byte_hi
    assert not (win.alias_slots & set(range(win.lo, win.hi)))
    row = h * d * es
    for slot in list(range(win.lo, win.lo + 2 * page)) + list(range(win.hi - 2 * page, win.hi)) + list(range(win.lo, win.hi, 37)):
        for off, part, rest in _element_offsets(name, slot):
            assert start <= off < start + span and start <= part, (slot, off, part)
            assert win.byte_lo <= off * es < win.byte_hi
            wrong = _truncations(off, part, rest, es) - {off * es}
            assert wrong, "no truncation changes this offset"
            for t in wrong:
                assert 0 <= base + t < bp.NBYTES - es, (name, slot, t)
                assert any(lo <= base + t < hi for lo, hi in ranges), (name, slot, t)
                if t >= 0:  # ... and the view's slots there (the whole page: an HND page interleaves its slots)
                    pg = t // (row * page)
                    assert set(range(pg * page, (pg + 1) * page)) <= win.alias_slots


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("name", sorted(bp.GEOMETRIES))
def test_high_window_truncations_stay_inside_the_storage(name, base):
    es = bp.GEOMETRIES[name][2]
    win = bp.geometry_window(name)
    _check(name, win, base, bp.TWO32, bp.TWO31 if es == 1 else 1 << 30)
    assert win.byte_lo >= bp.TWO32 * es  # every high slot's offset is >= 2^32 elements


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("name", ["bf16_h8_d128", "bf16_h2_d128"])
def test_mid_window_truncations_stay_inside_the_storage(name, base):
    """Offsets in [2^31, 2^31 + 2^20) elements of a view at storage byte MID_BASE: a signed 32-bit element offset is
    offset - 2^32 elements (below the view, inside the storage), a 32-bit byte offset is offset - 2^32 bytes."""
    h, d, es, page, layout = bp.GEOMETRIES[name]
    win = bp.mid_window(h * d, es, page, layout)
    _check(name, win, bp.MID_BASE + base, bp.TWO31, 1 << 20)
    assert sorted(win.alias) == [(win.byte_lo - 2 * bp.TWO32, win.byte_hi - 2 * bp.TWO32), (win.byte_lo - bp.TWO32, win.byte_hi - bp.TWO32)]
    assert min(lo for lo, _ in win.alias) < 0 <= bp.MID_BASE + base + min(lo for lo, _ in win.alias)


def test_k_and_v_windows_and_aliases_are_disjoint():
    for name in bp.GEOMETRIES:
        win = bp.geometry_window(name)
        k = [(lo, hi) for lo, hi in win.alias] + [(win.byte_lo, win.byte_hi)]
        v = [(bp.V_OFFSET + lo, bp.V_OFFSET + hi) for lo, hi in k]
        for (a, b), (c, e) in ((x, y) for x in k for y in v):
            assert b <= c or e <= a, (name, (a, b), (c, e))


@pytest.mark.parametrize("name", ["mx4_h2_d128", "mx4_mla"])
def test_scale_views_of_the_4_bit_pools_stay_clear_of_every_window_and_alias(name):
    h, d, es, page, layout = bp.GEOMETRIES[name]
    win = bp.geometry_window(name)
    srow = h * d // 8   # D / 16 scale bytes per head, D = 2 * d data bytes
    used = []
    for which in (0, 1):
        (v_lo, v_hi), (w_lo, w_hi), guards = bp.scale_ranges(which, srow, win)
        assert 0 <= v_lo <= guards[0][0] < w_lo < w_hi == v_hi <= guards[1][0] < guards[1][1] <= bp.NBYTES
        assert w_hi - w_lo == (win.hi - win.lo) * srow and w_hi < bp.TWO32   # (below 2^32: nothing to truncate)
        used.append((guards[0][0], guards[1][1]))
    assert used[0][1] <= used[1][0]
    for other in bp.GEOMETRIES:   # no data window, and no alias of one, reaches into the scale bytes
        ow = bp.geometry_window(other)
        for base in BASES:
            for lo, hi in [(ow.byte_lo, ow.byte_hi)] + list(ow.alias):
                assert all(base + hi <= a or base + lo >= b for a, b in used), (name, other)


# ---- the bounds the kernels assume are refused on the host -----------------------------------------------------------
def _refused(status, l):
    return status == -1 and b"2^31" in l.rx_last_error()


@pytest.mark.parametrize("field", ["k_page_stride", "k_tok_stride", "v_page_stride", "v_tok_stride"])
@pytest.mark.parametrize("value", [1 << 31, (1 << 32) + 4096, -8])
def test_attention_entries_refuse_strides_their_32_bit_multiplies_cannot_hold(field, value):
    """A stride is only a number: no pool that large is needed, and the check comes before any pointer is looked at
    (every buffer below is NULL), let alone a launch.  2^31 - 8 passes this check and fails the next one (null q / o)."""
    import ctypes as C

    from sglang_amd import lib

    l = lib.load()
    for make, call in ((lib.RxDecodeParams, lambda p: l.rx_decode_attn(C.byref(p), None)),
                       (lib.RxExtendParams, lambda p: l.rx_extend_attn(C.byref(p), None)),
                       (lib.RxDecodeParams, lambda p: l.rx_decode_attn_mx4(C.byref(p), C.byref(lib.RxKvMx4Scales()), None)),
                       (lib.RxExtendParams, lambda p: l.rx_extend_attn_mx4(C.byref(p), C.byref(lib.RxKvMx4Scales()), None))):
        p = make()
        p.bs, p.kv.page_size = 1, 16
        if make is lib.RxExtendParams:
            p.max_extend_len = 1
        setattr(p.kv, field, value)
        assert _refused(call(p), l), (make.__name__, l.rx_last_error())
        setattr(p.kv, field, (1 << 31) - 8)
        assert call(p) == -1 and b"2^31" not in l.rx_last_error() and b"null" in l.rx_last_error()


def test_extend_rows_and_scale_strides_are_bounded_too():
    import ctypes as C

    from sglang_amd import lib

    l = lib.load()
    for field in ("k_stride_t", "v_stride_t"):
        p = lib.RxExtendParams()
        p.bs, p.max_extend_len, p.kv.page_size = 1, 1, 1
        setattr(p, field, 1 << 31)
        assert _refused(l.rx_extend_attn(C.byref(p), None), l)
        assert _refused(l.rx_extend_attn_mx4(C.byref(p), C.byref(lib.RxKvMx4Scales()), None), l)
        p.unified_prefix_lens = 8   # (never read: q / o are null) -- the unified form has no k_extend / v_extend rows
        assert l.rx_extend_attn(C.byref(p), None) == -1 and b"null" in l.rx_last_error()
    for field in ("k_page_stride", "k_tok_stride", "v_page_stride", "v_tok_stride"):
        sc = lib.RxKvMx4Scales()
        setattr(sc, field, 1 << 31)
        d, e = lib.RxDecodeParams(), lib.RxExtendParams()
        d.bs = e.bs = e.max_extend_len = 1
        d.kv.page_size = e.kv.page_size = 1
        assert _refused(l.rx_decode_attn_mx4(C.byref(d), C.byref(sc), None), l)
        assert _refused(l.rx_extend_attn_mx4(C.byref(e), C.byref(sc), None), l)
