"""Device-free companion of test_gpu_wordwise_lists.py: the word-wise scheme of toed_compact_phase_kernel and
toed_need_compact_kernel (one wave per grid row, a lane per word of flags), transcribed into numpy lane for lane, gives the
arrays of the plain per-flag definition -- ranks, phase lists, list lengths, the `cap` guards and the `over` rule -- on random
flag rows and bitmaps, at the widths where a lane, a turn or the bitmap's second turn begins or ends."""
import numpy as np
import pytest

LANES = 64
EMPTY = -7  # what an array holds where nothing was stored


# ---- the pieces the two kernels share ---------------------------------------------------------------------------------
def wave_sum4(a):
    """a: [64, 4] per-lane partial sums -> the four sums, as every lane sees them."""
    return a.sum(axis=0, dtype=np.int64).astype(np.int32)


def wave_excl_scan_pair(x):
    """x: [64] uint32, even | odd << 16 -> (packed sums of the lanes in front, packed total); row shifts within the rows of
    16 lanes, then the row totals of the rows in front."""
    v = x.astype(np.uint32).copy()
    lane = np.arange(LANES)
    for d in (1, 2, 4, 8):
        sh = np.zeros_like(v)
        ok = (lane & 15) >= d
        sh[ok] = v[lane[ok] - d]
        v = v + sh
    t = [v[15], v[31], v[47], v[63]]
    row = lane >> 4
    front = np.where(row > 0, t[0], 0) + np.where(row > 1, t[1], 0) + np.where(row > 2, t[2], 0)
    return (v + front.astype(np.uint32) - x).astype(np.uint32), np.uint32(t[0] + t[1] + t[2] + t[3])


def walk_set_bits(m, emit):
    """emit(lanes, bits) for the lowest set bit of every lane that has one, until no lane has a bit left."""
    m = m.astype(np.uint32).copy()
    while (m != 0).any():
        on = np.nonzero(m)[0]
        low = m[on] & (~m[on] + np.uint32(1))
        emit(on, np.log2(low.astype(np.float64)).astype(np.int64))
        m[on] &= m[on] - np.uint32(1)


def popc(v):
    return np.unpackbits(np.ascontiguousarray(v, dtype="<u4").view(np.uint8).reshape(-1, 4), axis=1).sum(axis=1).astype(np.uint32)


def bytes_to_mask(b8):
    """[n, 8] flag bytes -> [n] 8-bit masks of the non-zero bytes, by the kernel's integer steps on two 32-bit halves."""
    w = np.ascontiguousarray(b8, dtype=np.uint8).view("<u4").astype(np.uint64)  # [n, 2]
    t = ((((w & 0x7F7F7F7F) + 0x7F7F7F7F) | w) >> 7) & 0x01010101
    nib = (((t * 0x01020408) & 0xFFFFFFFF) >> 24).astype(np.uint32)
    assert (nib < 16).all()
    return nib[:, 0] | (nib[:, 1] << 4)


# ---- toed_compact_phase_kernel ----------------------------------------------------------------------------------------
def compact_phase_naive(flag, cap):
    """Flag by flag in raster order: candidate r is the r-th flagged interior point, and goes to the end of its phase's list."""
    H2, W2 = flag.shape
    src = np.full(2 * cap, EMPTY, np.int64)
    lists = np.full((4, cap), EMPTY, np.int64)
    n = np.zeros(4, np.int64)
    ii, jj = np.nonzero(flag[10:H2 - 10, 10:W2 - 10])  # row-major
    r = 0
    for i, j in zip((ii + 10).tolist(), (jj + 10).tolist()):
        ph = ((i & 1) << 1) | (j & 1)
        if r < cap:
            src[2 * r], src[2 * r + 1] = i * W2 + j, -1
            lists[ph, n[ph]] = r
        r += 1
        n[ph] += 1
    over = r > cap
    counts = {2: 0 if over else r, 3: 0, 4: r}
    lcount = np.concatenate([np.zeros(4, np.int64) if over else n, np.zeros(8, np.int64)])
    return src, lists, counts, lcount


def compact_phase_wordwise(flag, cap):
    H2, W2 = flag.shape
    flat = flag.reshape(-1)  # the allocation: a load may not leave it
    inner = flag[:, 10:W2 - 10] != 0
    cnt = np.zeros((2, H2), np.int32)  # what the screen leaves in row_cnt: candidates in even / odd columns
    cnt[0, 10:H2 - 10] = inner[10:H2 - 10, 0::2].sum(axis=1)
    cnt[1, 10:H2 - 10] = inner[10:H2 - 10, 1::2].sum(axis=1)
    src = np.full(2 * cap, EMPTY, np.int64)
    lists = np.full(4 * cap, EMPTY, np.int64)
    counts, lcount = {}, np.full(12, EMPTY, np.int64)
    lane = np.arange(LANES)

    def sum_rows(r_end):
        a = np.zeros((LANES, 4), np.int32)
        for r0 in range(0, r_end, LANES):
            r = r0 + lane
            ok = r < r_end
            se = np.where(ok, cnt[0, np.minimum(r, H2 - 1)], 0)
            so = np.where(ok, cnt[1, np.minimum(r, H2 - 1)], 0)
            a[:, 0] += np.where(lane & 1, 0, se)
            a[:, 1] += np.where(lane & 1, 0, so)
            a[:, 2] += np.where(lane & 1, se, 0)
            a[:, 3] += np.where(lane & 1, so, 0)
        return wave_sum4(a)

    for blk in range((H2 - 20 + 3) // 4):
        for wv in range(4):
            i = 10 + 4 * blk + wv
            if i >= H2 - 10:
                continue
            pre = sum_rows(i)
            if i == 10:
                tot = sum_rows(H2)
                total = int(tot.sum())
                over = total > cap
                counts = {2: 0 if over else total, 3: 0, 4: total}
                lcount[:4] = 0 if over else tot
                lcount[4:] = 0
            base_all = int(pre.sum())
            base_e, base_o = int(pre[(i & 1) * 2]), int(pre[(i & 1) * 2 + 1])
            list_e = ((i & 1) << 1) * cap
            ncol = W2 - 20
            for c0 in range(0, ncol, 512):
                c = c0 + 8 * lane
                mask = np.zeros(LANES, np.uint32)
                on = np.nonzero(c < ncol)[0]
                first = i * W2 + 10 + c[on]
                assert (first + 8 <= (i + 1) * W2).all() and (first + 8 <= flat.size).all()  # inside the row, so inside the array
                assert (first % 2 == 0).all()                                              # bit parity = column parity
                m = bytes_to_mask(flat[first[:, None] + np.arange(8)])
                left = ncol - c[on]
                m = np.where(left < 8, m & ((np.uint32(1) << np.minimum(left, 8).astype(np.uint32)) - 1), m)
                mask[on] = m
                pe, po = popc(mask & 0x55), popc(mask & 0xAA)
                assert pe.sum() <= 256 and po.sum() <= 256
                front, total = wave_excl_scan_pair(pe | (po << 16))
                fe, fo = (front & 0xFFFF).astype(np.int64), (front >> 16).astype(np.int64)
                st = {"r": base_all + fe + fo, "e": base_e + fe, "o": base_o + fo}
                o0 = i * W2 + 10 + c

                def emit(ls, b):
                    par = b & 1
                    r = st["r"][ls]
                    ok = r < cap
                    src[2 * r[ok]] = o0[ls][ok] + b[ok]
                    src[2 * r[ok] + 1] = -1
                    pos = np.where(par, st["o"][ls], st["e"][ls]) + np.where(par, cap, 0)
                    lists[list_e + pos[ok]] = r[ok]
                    st["r"][ls] += 1
                    st["o"][ls] += par
                    st["e"][ls] += par ^ 1

                walk_set_bits(mask, emit)
                base_all += int(total & 0xFFFF) + int(total >> 16)
                base_e += int(total & 0xFFFF)
                base_o += int(total >> 16)
    return src, lists.reshape(4, cap), counts, lcount


def _flags(rng, H, W, density):
    f = (rng.random((2 * H, 2 * W)) < density).astype(np.uint8)
    odd = rng.random(f.shape) < 0.25  # any non-zero byte is a flag, not only 1
    f[(f != 0) & odd] = rng.choice(np.array([2, 0x80, 0xFF, 0x10], np.uint8), size=int(((f != 0) & odd).sum()))
    return f


# 2W - 20 = 10, 16 (a partial first lane, a whole number of lanes), 510, 512, 514 (the end of the first turn), 1024, 1026
COMPACT_W = [15, 18, 265, 266, 267, 522, 523]
DENSITIES = [0.0, 0.01, 0.07, 0.5, 1.0]


@pytest.mark.parametrize("W", COMPACT_W)
@pytest.mark.parametrize("H", [24, 25])
def test_compact_phase_wordwise_equals_per_flag(H, W):
    rng = np.random.default_rng(1000 * H + W)
    for density in DENSITIES:
        flag = _flags(rng, H, W, density)
        total = int((flag[10:2 * H - 10, 10:2 * W - 10] != 0).sum())
        assert total > 0 or density < 0.05
        for cap in sorted({max(total - 3, 1), max(total, 1), total + 5, max(total // 2, 1)}):
            want = compact_phase_naive(flag, cap)
            got = compact_phase_wordwise(flag, cap)
            where = (H, W, density, cap, total)
            assert np.array_equal(got[0], want[0]), where
            assert np.array_equal(got[1], want[1]), where
            assert got[2] == want[2], where
            assert np.array_equal(got[3], want[3]), where
            if total > cap:  # the `over` rule: lists published empty, the real total kept
                assert got[2][2] == 0 and got[2][4] == total and not got[3].any()


def test_compact_phase_one_column_parity_only():
    """Dense runs in one word, candidates in one column parity only (what a vertical step leaves)."""
    H, W = 24, 266
    flag = np.zeros((2 * H, 2 * W), np.uint8)
    flag[:, 300:340:2] = 1
    flag[20:24, 11::2] = 1
    for cap in (50, 10 ** 6):
        want, got = compact_phase_naive(flag, cap), compact_phase_wordwise(flag, cap)
        assert all(np.array_equal(g, w) for g, w in ((got[0], want[0]), (got[1], want[1]), (got[3], want[3]))) and got[2] == want[2]


# ---- toed_need_compact_kernel -----------------------------------------------------------------------------------------
def need_compact_naive(bits, W2, cap):
    H2 = bits.shape[0]
    lists = np.full((4, cap), EMPTY, np.int64)
    n = np.zeros(4, np.int64)
    on = np.unpackbits(np.ascontiguousarray(bits, dtype="<u4").view(np.uint8), axis=1, bitorder="little")[:, :W2]
    for I, J in zip(*(a.tolist() for a in np.nonzero(on))):  # bit by bit, row-major
        ph = ((I & 1) << 1) | (J & 1)
        if n[ph] < cap:
            lists[ph, n[ph]] = I * W2 + J
        n[ph] += 1
    return lists, n, int(n.sum())


def need_compact_wordwise(bits, W2, cap):
    H2, wpr = bits.shape
    assert wpr == (W2 + 31) >> 5
    ev, od = np.uint32(0x55555555), np.uint32(0xAAAAAAAA)
    cnt = np.stack([np.array([popc(bits[I] & ev).sum() for I in range(H2)]),
                    np.array([popc(bits[I] & od).sum() for I in range(H2)])]).astype(np.int32)  # toed_need_count_kernel
    lists = np.full(4 * cap, EMPTY, np.int64)
    lcount = np.full(4, EMPTY, np.int64)
    counts3 = 0
    lane = np.arange(LANES)
    for blk in range((H2 + 3) // 4):
        for wv in range(4):
            I = 4 * blk + wv
            if I >= H2:
                continue
            last = I >= H2 - 2
            mine0, mine1 = int(cnt[0, I]), int(cnt[1, I])
            if not last and mine0 + mine1 == 0:
                continue
            a = np.zeros((LANES, 4), np.int32)
            for r0 in range(I & 1, I, 128):
                r = r0 + 2 * lane
                ok = r < I
                a[:, 0] += np.where(ok, cnt[0, np.minimum(r, H2 - 1)], 0)
                a[:, 1] += np.where(ok, cnt[1, np.minimum(r, H2 - 1)], 0)
            s = wave_sum4(a)
            base_e, base_o = int(s[0]), int(s[1])
            if last:
                lcount[2 * (I & 1)], lcount[2 * (I & 1) + 1] = base_e + mine0, base_o + mine1
                counts3 += base_e + mine0 + base_o + mine1
            if mine0 + mine1 == 0:
                continue
            list_e = ((I & 1) << 1) * cap
            for k0 in range(0, wpr, LANES):
                k = k0 + lane
                v = np.where(k < wpr, bits[I, np.minimum(k, wpr - 1)], 0).astype(np.uint32)
                left = W2 - 32 * k
                v = np.where(left < 32, np.where(left > 0, v & ((np.uint32(1) << np.clip(left, 0, 31).astype(np.uint32)) - 1), 0), v)
                pe, po = popc(v & ev), popc(v & od)
                assert pe.sum() < 65536 and po.sum() < 65536
                front, total = wave_excl_scan_pair(pe | (po << 16))
                st = {"e": base_e + (front & 0xFFFF).astype(np.int64), "o": base_o + (front >> 16).astype(np.int64)}
                o0 = I * W2 + 32 * k

                def emit(ls, b):
                    par = b & 1
                    pos = np.where(par, st["o"][ls], st["e"][ls])
                    ok = pos < cap
                    lists[list_e + pos[ok] + np.where(par[ok], cap, 0)] = o0[ls][ok] + b[ok]
                    st["o"][ls] += par
                    st["e"][ls] += par ^ 1

                walk_set_bits(v, emit)
                base_e += int(total & 0xFFFF)
                base_o += int(total >> 16)
    return lists.reshape(4, cap), lcount, counts3


def _bitmap(rng, H, W, density):
    H2, W2 = 2 * H, 2 * W
    on = rng.random((H2, ((W2 + 31) >> 5) * 32)) < density
    on[:, W2:] = False  # columns >= 2W do not exist
    return np.packbits(on, axis=1, bitorder="little").view("<u4").astype(np.uint32), W2


# ceil(2W / 32) = 2, 3 and 63, 64, 65: the bitmap's first turn partly filled, full, and a second turn of one word
NEED_W = [32, 33, 1008, 1024, 1025]


@pytest.mark.parametrize("W", NEED_W)
@pytest.mark.parametrize("H", [24, 25])
def test_need_compact_wordwise_equals_per_bit(H, W):
    rng = np.random.default_rng(7000 * H + W)
    for density in DENSITIES:
        bits, W2 = _bitmap(rng, H, W, density)
        if density == 0.07:
            bits[2 * H - 2:] = 0  # the last two rows publish the lengths even when they are empty themselves
        _, n, total = need_compact_naive(bits, W2, 1)
        longest = int(n.max())
        for cap in sorted({max(longest - 3, 1), max(longest, 1), longest + 5, max(longest // 2, 1)}):
            want = need_compact_naive(bits, W2, cap)
            got = need_compact_wordwise(bits, W2, cap)
            where = (H, W, density, cap, longest)
            assert np.array_equal(got[0], want[0]), where
            assert np.array_equal(got[1], want[1]), where  # the lengths are the real ones, also past `cap`
            assert got[2] == want[2] == total, where


def test_scan_and_bit_walk_pieces():
    rng = np.random.default_rng(5)
    for _ in range(20):
        pe, po = rng.integers(0, 17, LANES).astype(np.uint32), rng.integers(0, 17, LANES).astype(np.uint32)
        front, total = wave_excl_scan_pair(pe | (po << 16))
        assert np.array_equal(front & 0xFFFF, np.concatenate([[0], np.cumsum(pe)[:-1]]))
        assert np.array_equal(front >> 16, np.concatenate([[0], np.cumsum(po)[:-1]]))
        assert total == pe.sum() | (po.sum() << 16)
    b = rng.integers(0, 256, (4096, 8)).astype(np.uint8)
    b[rng.random(b.shape) < 0.5] = 0
    assert np.array_equal(bytes_to_mask(b), ((b != 0) << np.arange(8)).sum(axis=1))
    m = rng.integers(0, 2 ** 32, LANES, dtype=np.uint64).astype(np.uint32)
    seen = [[] for _ in range(LANES)]
    walk_set_bits(m, lambda ls, bs: [seen[l].append(int(x)) for l, x in zip(ls, bs)])
    for l in range(LANES):
        assert seen[l] == [k for k in range(32) if (int(m[l]) >> k) & 1]
