"""-m gpu: the LDS-staged table kernel (csrc/gs360_tablestage.hip) at the limits of its own geometry, every byte against the CPU oracle:
every tile box the LDS budget admits (up to 766 16-byte chunks wide), boxes of exactly the budget and one chunk past it, the auto rule at its
threshold, sources with padded strides and offset base pointers, and calls of more than GS360_MAX_VIEWS (16) jobs.

The maps are designed tile by tile from a host model of the stage plan (`plan_model`).  Output widths are multiples of 64 and positions
exact multiples of 1/32 px, so tile (tx, ty) is exactly output pixels [64 tx, 64 tx + 64) x [R ty, R ty + R) and the map plan's
quantisation is known."""
import ctypes as C

import numpy as np
import pytest

import gs360

pytestmark = pytest.mark.gpu

BUDGET = 26 * 1024 - 64                   # kTsBoxBudget (csrc/gs360_capi_remap.hip:85): largest box in bytes
BUDGET_CHUNKS = BUDGET // 16              # 1660
MAX_DIM = gs360.Context.MAP_PLAN_MAX_DIM  # 4079: the widest source a map plan addresses
FAST, FILL, BORDER, SLOW = -1, 0, 1, 2    # ts_classify's kinds


def _diff(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        d = np.abs(got.astype(int) - want.astype(int))
        raise AssertionError(f"{what}: {len(bad)} mismatching bytes of {got.size}, max |d| = {d.max()}, first at {bad[0].tolist()}")


# ---- host model of table_stage_plan_kernel (csrc/gs360_tablestage.hip) -------------------------------------------------------------------
def wch_of(minx, maxx):
    """16-byte chunks per box row of a tile whose fast taps span columns minx..maxx (gs360_tablestage.hip:108-109)"""
    x0b = (3 * minx) & ~15
    return ((((3 * maxx - x0b) & ~3) + 12) + 15) >> 4


def plan_model(mx, my, W, H, R, valid=None):
    """the stage plan of maps mx, my (h x w, w % 64 == 0) for a W x H source and tiles of R rows: per tile whether it has fast pixels, its
    box's wch and nrows, and whether the box fits the budget.  Quantisation: map_pack_kernel (gs360_table.hip:31-37), kinds: ts_classify
    (gs360_tablestage.hip:59-72), box: :104-116, tiles: ts_build_plan (:394-395)."""
    h, w = mx.shape
    assert w % 64 == 0
    sx = np.rint(mx.astype(np.float32) * np.float32(32)).astype(np.int64)
    sy = np.rint(my.astype(np.float32) * np.float32(32)).astype(np.int64)
    ix, iy = np.clip(sx >> 5, -8, MAX_DIM + 8), np.clip(sy >> 5, -8, MAX_DIM + 8)
    fx, fy = sx & 31, sy & 31
    kind = np.full((h, w), SLOW, np.int8)
    kind[(ix >= 0) & (iy >= 0) & ((ix <= W - 2) | ((ix == W - 1) & (fx == 0))) & ((iy <= H - 2) | ((iy == H - 1) & (fy == 0)))] = FAST
    kind[(ix >= W) | (ix + 1 < 0) | (iy >= H) | (iy + 1 < 0)] = BORDER
    if valid is not None:
        kind[~np.asarray(valid, bool)] = FILL
    tiles_x, tiles_y = (w + 3 + 63) // 64, (h + R - 1) // R        # (the last tile column of a w % 64 == 0 output holds no pixel)
    fast = np.zeros((tiles_y * R, tiles_x * 64), bool)
    fast[:h, :w] = kind == FAST
    big = 1 << 30

    def reduce(a, fn, empty):
        full = np.full(fast.shape, empty, np.int64)
        full[:h, :w] = a
        full[~fast] = empty
        return fn(full.reshape(tiles_y, R, tiles_x, 64), axis=(1, 3)).ravel()
    minx, maxx = reduce(ix, np.min, big), reduce(ix, np.max, -1)
    miny, maxy = reduce(iy, np.min, big), reduce(iy, np.max, -1)
    has = maxx >= 0
    wch = np.where(has, wch_of(np.where(has, minx, 0), np.where(has, maxx, 0)), 0)
    nrows = np.where(has, maxy - miny + 2, 0)
    boxed = has & (nrows * wch * 16 <= BUDGET)
    return dict(n_tiles=tiles_x * tiles_y, tiles_x=tiles_x, has=has, wch=wch, nrows=nrows, boxed=boxed,
                slow_tiles=int((has & ~boxed).sum()), kind=kind)


# ---- map design --------------------------------------------------------------------------------------------------------------------------
_feasible_cache = {}


def _feasible_minx(wch, W):
    """columns minx from which a box of exactly wch chunks exists inside a W-wide source, and for each the rightmost maxx that gives it"""
    key = (wch, W)
    if key not in _feasible_cache:
        minx = np.arange(W, dtype=np.int64)
        x0b = (3 * minx) & ~15
        maxx = np.minimum((x0b + 16 * wch - 9) // 3, W - 1)       # ((d & ~3) + 27) >> 4 <= wch  <=>  d <= 16 wch - 9
        ok = (maxx >= minx) & (wch_of(minx, maxx) == wch)
        _feasible_cache[key] = (minx[ok], maxx[ok])
    return _feasible_cache[key]


def max_wch(W):
    return int(wch_of(0, W - 1))


def box_for(rng, wch, nrows, W, H, phase, clamp_bottom, reach_right=False):
    """(minx, maxx, miny, maxy) of a box of wch x nrows chunks: 3 minx mod 16 == phase where the width allows; maxx is the rightmost column
    that keeps wch -- W - 1 if reach_right (or if only W - 1 gives wch), else short of it, so that taps with weight read the box's last
    chunk; clamp_bottom puts the last fast row on H - 1 (the box's bottom row is then clamped by the loader)"""
    mins, maxs = _feasible_minx(wch, W)
    assert len(mins), (wch, W)
    at_edge = maxs == W - 1
    if at_edge.any() and (reach_right or at_edge.all()):
        mins, maxs = mins[at_edge], maxs[at_edge]
    else:
        mins, maxs = mins[~at_edge], maxs[~at_edge]
    sel = np.flatnonzero((3 * mins) % 16 == phase % 16)
    k = int(rng.choice(sel)) if len(sel) else int(rng.integers(len(mins)))
    minx, maxx = int(mins[k]), int(maxs[k])
    assert 2 <= nrows <= H + 1
    if clamp_bottom:
        maxy = H - 1
    else:
        maxy = int(rng.integers(nrows - 2, H - 1)) if nrows - 2 < H - 1 else H - 1
    return minx, maxx, maxy - (nrows - 2), maxy


def tile_positions(rng, npix, box, W, H):
    """npix fast positions (x, y: multiples of 1/32) whose box is exactly `box`: its two corners, several pixels on the last 1-6 texels of
    every box row (fx != 0, fy != 0: they read the box rows' last bytes), a weight-zero tap on W - 1 where the box reaches it, and random
    positions inside the box for the rest"""
    minx, maxx, miny, maxy = box
    xe = min(maxx, W - 2)                                # the rightmost column a tap with fx != 0 may use
    ix, iy = [np.array([minx, maxx, W - 1][:3 if maxx == W - 1 else 2])], [np.array([miny, maxy, maxy])[:3 if maxx == W - 1 else 2]]
    if xe >= minx:
        rows = np.arange(miny, maxy + 1)
        if len(rows) > npix // 2:                        # taller boxes than half the tile's pixels: a spread of rows, first and last included
            rows = np.unique(np.linspace(miny, maxy, npix // 2).astype(np.int64))
        per = max(1, min(6, (npix // 2) // len(rows), xe - minx + 1))
        ix.append(np.tile(xe - np.arange(per), len(rows)))
        iy.append(np.repeat(rows, per))
    n_fixed = sum(len(a) for a in ix)
    n_rest = npix - n_fixed
    assert n_rest >= 0
    ix = np.concatenate(ix + [rng.integers(minx, max(xe, minx) + 1, n_rest)]).astype(np.int64)
    iy = np.concatenate(iy + [rng.integers(miny, maxy + 1, n_rest)]).astype(np.int64)
    fx = rng.integers(0, 32, npix)
    fy = rng.integers(0, 32, npix)
    fx[1:n_fixed] = rng.integers(1, 32, n_fixed - 1)     # (the corner at minx may have fx = 0; all others carry weight on the right / bottom)
    fy[1:n_fixed] = rng.integers(1, 32, n_fixed - 1)
    fx[ix == W - 1] = 0                                  # the last column / row only with weight-zero right / bottom taps: still fast
    fy[iy == H - 1] = 0
    perm = rng.permutation(npix)
    return (ix[perm] + fx[perm] / 32.0).astype(np.float32), (iy[perm] + fy[perm] / 32.0).astype(np.float32)


def design_maps(rng, pairs, W, H, R, tiles_per_row, h=None, clamp=lambda t: t % 5 == 2, reach=lambda t: t % 4 == 1):
    """maps whose tiles, in order, have boxes of pairs[i] = (wch, nrows) chunks; tiles past the list repeat it from the start.  Tile t's
    box ends on row H - 1 where clamp(t) (its last box row is then read with weight zero only) and on column W - 1 where reach(t) and its
    width allow (its last chunks then hold texels past the image, read with weight zero only).  Returns (mx, my, designed (wch, nrows) per
    model tile or None)."""
    n_rows_t = (len(pairs) + tiles_per_row - 1) // tiles_per_row
    h = h or n_rows_t * R
    w = 64 * tiles_per_row
    mx = np.empty((h, w), np.float32)
    my = np.empty((h, w), np.float32)
    tiles_x = (w + 3 + 63) // 64
    designed = [None] * (tiles_x * ((h + R - 1) // R))
    t = 0
    for ty in range((h + R - 1) // R):
        rr = min(R, h - R * ty)
        for tx in range(tiles_per_row):
            wch, nrows = pairs[t % len(pairs)]
            box = box_for(rng, wch, nrows, W, H, phase=t, clamp_bottom=clamp(t) and nrows <= H + 1, reach_right=reach(t))
            px, py = tile_positions(rng, 64 * rr, box, W, H)
            mx[R * ty:R * ty + rr, 64 * tx:64 * tx + 64] = px.reshape(rr, 64)
            my[R * ty:R * ty + rr, 64 * tx:64 * tx + 64] = py.reshape(rr, 64)
            designed[ty * tiles_x + tx] = (wch, nrows)
            t += 1
    return mx, my, designed


def check_design(model, designed):
    """the model finds every designed box (a self-check of the design code, before the GPU is asked)"""
    for t, d in enumerate(designed):
        if d is None:
            assert not model["has"][t], t
        else:
            assert (int(model["wch"][t]), int(model["nrows"][t])) == d, (t, d, int(model["wch"][t]), int(model["nrows"][t]))


def bad_tiles(got, want, R, tiles_x, designed):
    """designed (wch, nrows) of the tiles holding mismatching pixels"""
    yy, xx = np.nonzero((got != want).any(axis=2))
    ids = np.unique((yy // R) * tiles_x + xx // 64)
    return sorted({designed[i] for i in ids.tolist()})


# ---- fixtures and launch helpers ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide_src(ctx):
    """a 4079 x 1700 random source: the widest a map plan addresses, taller than the tallest box; rows of 12 240 bytes (3 W + 3: the
    staged kernel needs rows of whole dwords), junk in the padding -> (image, buffer, pointer, stride)"""
    img, buf, ptr = _source_case(ctx, np.random.default_rng(4079), MAX_DIM, 1700, 3 * MAX_DIM + 3, 0)
    yield img, buf, ptr, 3 * MAX_DIM + 3
    ctx.free(buf)


def _source_case(ctx, rng, W, H, stride, off):
    """a W x H RGB image at byte `off` of a device buffer, rows `stride` bytes apart, junk in the padding -> (image, buffer, pointer)"""
    raw = rng.integers(0, 256, off + H * stride, dtype=np.uint8)
    img = raw[off:].reshape(H, stride)[:, :3 * W].reshape(H, W, 3).copy()
    buf = ctx.to_device(raw)
    return img, buf, buf.ptr + off


def _plan(ctx, mx, my, valid=None):
    h, w = mx.shape
    d = [ctx.to_device(mx), ctx.to_device(my), ctx.to_device(np.asarray(valid, np.uint8)) if valid is not None else None]
    plan = ctx.map_plan(d[0], d[1], d[2], h, w)
    for b in d:
        if b is not None:
            ctx.free(b)
    return plan


def _raw_call(ctx, jobs, plans, bv):
    """gs360_remap_plans_u8 on RemapJob records -> (last_table_kernel, last_table_stage_slow_tiles)"""
    n = len(jobs)
    arr = (gs360.capi.RemapJob * n)(*jobs)
    pl = (C.c_void_p * n)(*plans)
    cbv = (C.c_double * 4)(*bv)
    gs360.capi._check(ctx.L.gs360_remap_plans_u8(ctx.handle, arr, pl, n, 3, 1, cbv, 0), ctx.L)
    ctx.sync(0)
    return ctx.get_option("last_table_kernel"), ctx.get_option("last_table_stage_slow_tiles")


def _run_one(ctx, source, mx, my, bv=(23.0, 140.0, 7.0, 0.0), **opts):
    """one job on `source` (image, buffer, pointer, stride) -> (output, last_table_kernel, last_table_stage_slow_tiles)"""
    img, _, ptr, stride = source
    H, W = img.shape[:2]
    h, w = mx.shape
    plan = _plan(ctx, mx, my)
    dst = ctx.alloc(h * w * 3)
    try:
        with ctx.options(**opts):
            staged, slow = _raw_call(ctx, [gs360.capi.RemapJob(ptr, H, W, stride, None, None, None, h, w, 0, dst.ptr, 0)], [plan], bv)
        return ctx.download(dst, (h, w, 3)), staged, slow
    finally:
        ctx.map_plan_free(plan)
        ctx.free(dst)


def sweep_pairs(thin=False):
    """every (wch, nrows) box the budget admits on a 4079-wide source; thin: nrows in {2, max} only"""
    out = []
    for wch in range(1, max_wch(MAX_DIM) + 1):
        top = BUDGET_CHUNKS // wch
        out += [(wch, 2), (wch, top)] if thin and top > 2 else ([(wch, 2)] if thin else [(wch, n) for n in range(2, top + 1)])
    return out


# ---- 1. every box shape ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [8, 24, 32])
def test_box_shape_sweep(ctx, orc, wide_src, rows):
    """one tile for every (wch, nrows) the budget admits (8-row tiles: all ~10 800 of them; 24 / 32 rows: every wch with two rows and the
    most the budget allows, output heights of k R + 1 so that the last tile row holds one pixel row), boxes as wide as a 4079-texel row
    allows, 3 minx mod 16 cycling, weighted taps on the last texels of every box row; then every wch with two rows and the most rows again,
    once with the bottom box row clamped (last fast row H - 1) and once ending on W - 1: all staged, none slow, every byte"""
    src = wide_src[0]
    H, W = src.shape[:2]
    assert max_wch(W) == 766
    main, var = sweep_pairs(thin=rows != 8), sweep_pairs(thin=True)
    pairs = main + var + var                             # every box with weight on all its bytes; then the thin set clamped at H - 1, and at W - 1
    n, m = len(main), len(var)
    per_row = 128
    n_rows_t = (len(pairs) + per_row - 1) // per_row
    h = n_rows_t * rows if rows == 8 else (n_rows_t - 1) * rows + 1
    rng = np.random.default_rng(700 + rows)
    mx, my, designed = design_maps(rng, pairs, W, H, rows, per_row, h=h, clamp=lambda t: n <= t < n + m, reach=lambda t: t >= n + m)
    model = plan_model(mx, my, W, H, rows)
    check_design(model, designed)
    assert model["slow_tiles"] == 0
    got, staged, slow = _run_one(ctx, wide_src, mx, my, table_stage=1, table_stage_rows=rows)
    want = orc.remap_u8(src, mx, my, interp=1, border_value=(23.0, 140.0, 7.0, 0.0), threads=0).reshape(got.shape)
    bad = bad_tiles(got, want, rows, model["tiles_x"], designed)
    assert not bad, f"rows={rows}: tiles of these (wch, nrows) boxes differ from the oracle: {bad}"
    assert staged == 1 and slow == 0, (staged, slow)


# ---- 2. the budget's edge ----------------------------------------------------------------------------------------------------------------
def test_budget_edge(ctx, orc, wide_src):
    """boxes of exactly 26 560 bytes (every factor pair of 1660 chunks) are staged, boxes one 16-byte chunk past it (1661 chunks) and more go
    the slow way: the slow-tile counter equals the model's count, every byte matches"""
    src = wide_src[0]
    H, W = src.shape[:2]
    exact = [(d, BUDGET_CHUNKS // d) for d in range(1, max_wch(W) + 1) if BUDGET_CHUNKS % d == 0 and BUDGET_CHUNKS // d >= 2]
    over = [(1, 1661), (11, 151), (151, 11), (2, 831), (83, 21), (766, 3), (415, 5)]
    assert (83, 20) in exact and all(a * b == BUDGET_CHUNKS + 1 for a, b in over[:3])
    rng = np.random.default_rng(26560)
    pairs = []
    for k in range(3):                                   # each edge case three times, with other columns / phases, among ordinary boxes
        pairs += exact + over + [(int(rng.integers(1, 200)), int(rng.integers(2, 8))) for _ in range(6)]
    mx, my, designed = design_maps(rng, pairs, W, H, 8, 8)
    model = plan_model(mx, my, W, H, 8)
    check_design(model, designed)
    n_over = sum(1 for d in designed if d is not None and d[0] * d[1] > BUDGET_CHUNKS)
    assert model["slow_tiles"] == n_over == 3 * len(over)
    got, staged, slow = _run_one(ctx, wide_src, mx, my, table_stage=1, table_stage_rows=8)
    want = orc.remap_u8(src, mx, my, interp=1, border_value=(23.0, 140.0, 7.0, 0.0), threads=0).reshape(got.shape)
    bad = bad_tiles(got, want, 8, model["tiles_x"], designed)
    assert not bad, f"tiles of these (wch, nrows) boxes differ from the oracle: {bad}"
    assert staged == 1
    assert slow == model["slow_tiles"], (slow, model["slow_tiles"])


# ---- 3. the auto rule at its threshold ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, 1])
def test_auto_rule_threshold(ctx, orc, wide_src, extra):
    """table_stage = -1 stages a plan whose over-budget tiles are exactly n_tiles / 8 and keeps the gather kernel with one more
    (gs360_capi_remap.hip:213); both outputs match every byte"""
    src = wide_src[0]
    H, W = src.shape[:2]
    rng = np.random.default_rng(88 + extra)
    per_row, R = 7, 8                                    # 7 tiles + the empty column: 8 per tile row; 8 tile rows: n_tiles = 64
    n_over = 64 // 8 + extra
    pairs = [(int(rng.integers(1, 300)), int(rng.integers(2, 6))) for _ in range(per_row * 8)]
    for k in rng.choice(len(pairs), n_over, replace=False):
        pairs[k] = (int(rng.integers(120, 700)), int(rng.integers(14, 40)))
    mx, my, designed = design_maps(rng, pairs, W, H, R, per_row)
    model = plan_model(mx, my, W, H, R)
    check_design(model, designed)
    assert model["n_tiles"] == 64 and model["slow_tiles"] == n_over
    got, staged, slow = _run_one(ctx, wide_src, mx, my, table_stage=-1, table_stage_rows=R)
    assert staged == (1 if extra == 0 else 0), staged
    assert slow == (n_over if extra == 0 else 0), slow
    want = orc.remap_u8(src, mx, my, interp=1, border_value=(23.0, 140.0, 7.0, 0.0), threads=0).reshape(got.shape)
    _diff(got, want, f"auto rule, {n_over} of 64 tiles over budget")


# ---- 4. sources as callers hand them over ------------------------------------------------------------------------------------------------
def _limit_pairs(rng, W, H, n):
    """boxes for a source of W x H: the widest with two rows and with the most rows, clamped-bottom ones, random others"""
    top = max_wch(W)
    base = [(top, 2), (top, min(BUDGET_CHUNKS // top, H + 1)), (top - 1, 2), (1, min(BUDGET_CHUNKS, H + 1))]
    while len(base) < n:
        wch = int(rng.integers(1, top + 1))
        base.append((wch, int(rng.integers(2, min(BUDGET_CHUNKS // wch, H + 1) + 1))))
    return base


def test_padded_and_offset_sources(ctx, orc):
    """src_stride = 3 W + 4 and + 64, an odd W with a padded stride that is a multiple of 4, a source 4 bytes into its buffer: staged; a
    source 1 byte into its buffer and strides that are not multiples of 4: the gather kernel, in the same call; every byte matches"""
    rng = np.random.default_rng(44)
    H, R = 300, 8
    cases = [  # (W, stride, offset, staged)
        (1000, 3004, 0, True), (1000, 3064, 0, True), (999, 3000, 0, True), (999, 3060, 0, True), (1000, 3000, 4, True),
        (1000, 3000, 1, False), (1000, 3002, 0, False), (999, 2997, 0, False), (1000, 3004, 2, False)]
    bv = (5.0, 250.0, 99.0, 0.0)
    jobs, plans, bufs, wants = [], [], [], []
    for k, (W, stride, off, _) in enumerate(cases):
        img, sbuf, sptr = _source_case(ctx, rng, W, H, stride, off)
        mx, my, designed = design_maps(rng, _limit_pairs(rng, W, H, 20), W, H, R, 5)
        check_design(plan_model(mx, my, W, H, R), designed)
        h, w = mx.shape
        plans.append(_plan(ctx, mx, my))
        dst = ctx.alloc(h * w * 3)
        ctx.memset(dst, 0xAB)
        bufs += [sbuf, dst]
        jobs.append(gs360.capi.RemapJob(sptr, H, W, stride, None, None, None, h, w, 0, dst.ptr, 0))
        wants.append((dst, orc.remap_u8(img, mx, my, interp=1, border_value=bv, threads=0).reshape(h, w, 3)))
    try:
        with ctx.options(table_stage=1, table_stage_rows=R):
            staged, slow = _raw_call(ctx, jobs, plans, bv)
        for k, ((W, stride, off, _), (dst, want)) in enumerate(zip(cases, wants)):
            _diff(ctx.download(dst, want.shape), want, f"source {W} wide, stride {stride}, offset {off}")
        assert staged == sum(c[3] for c in cases), staged
        assert slow == 0
    finally:
        for p in plans:
            ctx.map_plan_free(p)
        for b in bufs:
            ctx.free(b)


# ---- 5. calls of more than 16 jobs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_jobs", [17, 35])
def test_calls_of_more_than_16_jobs(ctx, orc, n_jobs):
    """17- and 35-job calls (two and three launches) under the auto rule: staged and ineligible jobs, one map plan used with two source sizes
    and with the valid fill on and off (stage plans keyed by (W, H, R, valid)), one source size at two strides (one stage plan).  The
    counters cover the whole call; every byte of every job matches; a second call on the cached stage plans gives the same bytes"""
    rng = np.random.default_rng(1600 + n_jobs)
    R, h, w = 8, 32, 512                                 # 9 x 4 = 36 tiles per plan: the auto rule stages plans with at most 4 slow tiles
    bv, fill = (17.0, 3.0, 201.0, 0.0), 77
    A = _source_case(ctx, rng, 1200, 300, 3600, 0)       # (image, buffer, pointer)
    A2 = _source_case(ctx, rng, 1200, 300, 3664, 0)      # the same size, another stride
    B = _source_case(ctx, rng, 640, 180, 1920, 0)        # the shared plan with a smaller source: other slow / border classes
    X = _source_case(ctx, rng, 1200, 300, 3600, 1)       # not dword-aligned: the gather kernel
    srcs = {"A": (A, 1200, 300, 3600), "A2": (A2, 1200, 300, 3664), "B": (B, 640, 180, 1920), "X": (X, 1200, 300, 3600)}

    def maps(n_over):
        pairs = _limit_pairs(rng, 1200, 300, 32)
        for k in rng.choice(len(pairs), n_over, replace=False):
            pairs[k] = (int(rng.integers(120, 220)), int(rng.integers(16, 40)))
        return design_maps(rng, pairs, 1200, 300, R, 8)[:2]
    shared = maps(3) + ((rng.random((h, w)) > 0.1),)     # 3 over-budget tiles of 36: staged under the auto rule
    others = [maps(int(rng.integers(0, 3))) + (None,) for _ in range(3)]
    scattered = maps(6) + (None,)                        # 6 of 36: the auto rule keeps the gather kernel
    maplist = [shared] + others + [scattered]
    plans = [_plan(ctx, mx, my, valid) for mx, my, valid in maplist]
    menu = [("A", 0, True), ("A", 0, False), ("B", 0, True), ("B", 0, False), ("A2", 0, True), ("A2", 0, False), ("X", 1, False),
            ("A", 4, False), ("A2", 1, False), ("B", 2, False), ("A", 3, False), ("X", 0, True), ("B", 4, False)]
    order = [menu[k % len(menu)] for k in range(n_jobs)]
    rng.shuffle(order)
    jobs, pls, dsts, wants = [], [], [], []
    want_staged = want_slow = 0
    cache = {}
    for s, m, use_valid in order:
        (img, _, ptr), W, H, stride = srcs[s]
        mx, my, valid = maplist[m]
        key = (s, m, use_valid)
        if key not in cache:
            want = orc.remap_u8(img, mx, my, interp=1, border_value=bv, threads=0).reshape(h, w, 3)
            if use_valid:
                want = orc.valid_fill(want.copy(), valid, fill)
            model = plan_model(mx, my, W, H, R, valid if use_valid else None)
            cache[key] = (want, model)
        want, model = cache[key]
        if s != "X" and model["slow_tiles"] * 8 <= model["n_tiles"]:
            want_staged += 1
            want_slow += model["slow_tiles"]
        dst = ctx.alloc(h * w * 3)
        dsts.append(dst)
        wants.append(want)
        jobs.append(gs360.capi.RemapJob(ptr, H, W, stride, None, None, dst.ptr if use_valid else None, h, w, fill, dst.ptr, 0))
        pls.append(plans[m])
    assert 0 < want_staged < n_jobs and want_slow > 0
    try:
        outs = []
        for turn in range(2):                            # the second call runs on the cached stage plans
            for d in dsts:
                ctx.memset(d, 0xAB)
            with ctx.options(table_stage=-1, table_stage_rows=R):
                staged, slow = _raw_call(ctx, jobs, pls, bv)
            outs.append([ctx.download(d, (h, w, 3)) for d in dsts])
            for k, (got, want) in enumerate(zip(outs[-1], wants)):
                _diff(got, want, f"{n_jobs}-job call {turn}, job {k} {order[k]}")
            assert (staged, slow) == (want_staged, want_slow), f"call {turn}: counters {(staged, slow)}, whole call {(want_staged, want_slow)}"
        assert all(np.array_equal(a, b) for a, b in zip(*outs))
    finally:
        for p in plans:
            ctx.map_plan_free(p)
        for b in dsts + [A[1], A2[1], B[1], X[1]]:
            ctx.free(b)
