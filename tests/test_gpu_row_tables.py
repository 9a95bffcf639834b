"""A region-statistics session and a localize session open on ONE context, their add_rows calls interleaved piece by piece: the two share the
host code behind the row sessions (the checks, the upload into each session's own buffer, the launch wrapper) and the device code of the
code-slot table, and each must give what it gives alone.  The fused runs of test_gpu_localize.py cover add_resident for both at once; this
is the upload path.  Shapes: 4097 rows (past one 4096-row stats chunk, several 256-row localize sweeps) cut into three pieces, 257 regions
(two localize batches), a window of two tiles, five codes (one beyond the four LDS slots), no fixed code list (both kernels claim slots)."""
import numpy as np
import pytest

import modkit_amd
import test_gpu_localize as loc
import test_gpu_region_stats as stats

pytestmark = pytest.mark.gpu

N_ROWS, N_REGIONS, WINDOW = 4097, 257, modkit_amd.localize_tile_offsets() // 2 + 1
CUTS = [(0, 1500), (1500, 3100), (3100, N_ROWS)]


def test_interleaved_sessions_on_one_context_equal_each_alone():
    rows = stats.make_rows(N_ROWS, seed=61, codes=stats.CODES16[:5])
    length = loc.contig_length(rows)
    pieces = [(0, {k: v[a:b] for k, v in rows.items()}) for a, b in CUTS]
    stats_regions = stats.make_regions(rows, N_REGIONS, seed=62)
    loc_regions = loc.make_regions(rows, N_REGIONS, seed=63, window=WINDOW)
    stats_alone = stats.device_totals(pieces, stats_regions)
    loc_alone = loc.device_counts(pieces, loc_regions, [length], WINDOW)
    ctx = modkit_amd.Context()
    try:
        ctx.stats_begin([(0, s, e, st) for _c, s, e, _n, st in stats_regions])
        ctx.localize_begin([(0, s, e, st) for _c, s, e, st in loc_regions], [length], window=WINDOW)
        for tid, piece in pieces:
            ctx.stats_add_rows(tid, piece)
            ctx.localize_add_rows(tid, piece)
        stats_both, loc_both = ctx.stats_get(), ctx.localize_get()
    finally:
        ctx.close()
    assert sorted(stats_both) == sorted(stats_alone) and sorted(loc_both) == sorted(loc_alone)
    for k in stats_alone:
        assert np.array_equal(stats_both[k], stats_alone[k]), k
    for k in loc_alone:
        assert np.array_equal(loc_both[k], loc_alone[k]), k
    # and what each gives alone is the model's (numpy form, pinned by the model in the two files the generators come from)
    assert len(stats_alone["codes"]) == len(loc_alone["codes"]) == 5
    stats.assert_same(stats_alone, stats.fast_totals(rows, stats_regions, None, 1), None)
    assert loc.cells_of(loc_alone) == loc.fast_counts(rows, loc_regions, length, WINDOW)
