"""The shapes of tests/test_gpu_readout_strides.py without a GPU: tests/stride_cases.py restates from the constants in the sources which loops of the
chunked read-outs a shape reaches, and every shape is held here to exactly the coverage it is there for — the second trip of a workgroup through the
tile loop of the value kernels, the pieces of LevelsSummary::run with their edges inside and between the rows' curves, the rounds of k_level_rows, the
launch counts the read-outs report.  A constant changed without moving the shapes fails here; the GPU tests then do not silently leave their loops.
The ambiguity share of the rows whose curves meet the model on the GPU is held under curve_cases.AMBIGUOUS_MAX from the model alone, on the emulated
layer's predict_bart."""
import numpy as np
import pytest

import curve_cases as cv
import stride_cases as st


@pytest.fixture(scope="module")
def c():
    return st.constants()


def test_constants_are_the_ones_the_shapes_were_chosen_for(c):
    assert (c["PS_BLOCK"], c["PS_GRID_MAX"], c["GP_SORT_LEVELS"], c["GRID_MAX"], c["BLOCK"], c["QT_SORT"]) == (1024, 1024, 1 << 20, 2048, 256, 4096)
    assert c["S4B_QT_SCRATCH_MIB"] == 64 and c["CV_SCRATCH_DEFAULT"] == 512 << 20
    assert st.big_rows(c) == 1048641 and st.small_rows(c) == 209780 and st.S == sum(st.POOL) == 3


def test_one_chunk_of_quantiles_contrast_and_groups_takes_workgroup_0_round_twice(c):
    N = st.big_rows(c)
    p = st.plan(N, st.S, c=c)
    assert (p["C"], p["chunks"], p["tiles"], p["workgroups"]) == (N, 1, c["PS_GRID_MAX"] + 1, c["PS_GRID_MAX"])
    assert p["trips_first"] == 2 and p["trips_last"] == 1          # workgroup 0 alone takes a second tile
    assert p["last_tile_rows"] == 65                               # a full wave and a wave with one live lane
    assert (p["Sp"], p["R"]) == (4, 1024)
    assert st.quantiles_launches(p) == 2
    assert st.contrast_launches(p, per_row=True, weights=2, probs=3) == 4
    # every row its own level: no level over a slab edge, 16 386 slabs (the last of one row), the sort of the level matrix in two pieces
    assert p["slabs"] == 16386
    lev = st.pieces(N, 1, c)
    assert lev["pieces"] == 2 and lev["edges"] == [(1 << 20, 0)]
    assert -(-N // (c["GRID_MAX"] * (c["BLOCK"] // 64))) == 129 and lev["level_rounds"] == 128          # (groups_run's own launch over all L: 129 rounds)
    assert st.groups_launches(p, N, probs=3, c=c) == 5
    assert 8 * N * st.S <= 1 << 30          # GROUPS_LEVEL_BYTES_MAX


def test_comparison_calls_stay_inside_one_grid_and_one_piece(c):
    N = st.big_rows(c)
    for G in (1, st.G_BIG):
        p = st.plan(N, st.S, G, st.compare_scratch(G), st.default_scratch("curves" if G > 1 else "quantiles", c), c)
        assert (p["C"], p["chunks"], p["last_chunk_rows"], p["tiles"]) == (1 << 18, 5, 65, 256)
        assert p["trips_first"] == p["trips_last"] == 1 and p["point"]["pieces"] == 1 and p["range"]["pieces"] == 1
    assert p["C"] * st.G_BIG == 786432
    assert st.curves_launches(p, st.G_BIG, probs=3, c=c) == 5 * 6 == 30
    p1 = st.plan(N, st.S, 1, st.compare_scratch(1), c=c)
    assert st.quantiles_launches(p1) == 10 and st.contrast_launches(p1, True, 2, 3) == 20 and st.groups_launches(p1, N, probs=3, c=c) == 13


def test_big_curves_shape_has_four_pieces_with_edges_inside_and_between_the_curves(c):
    N, G = st.big_rows(c), st.G_BIG
    p = st.plan(N, st.S, G, 0, st.default_scratch("curves", c), c)
    assert (p["C"], p["chunks"], p["tiles"], p["trips_first"], p["trips_last"], p["last_tile_rows"], p["slabs"]) == (N, 1, 1025, 2, 1, 65, 16386)
    assert p["C"] * G == 3145923 and p["point"]["pieces"] == 4 and p["range"]["pieces"] == 2
    assert p["point"]["edges"] == [(349525, 1), (699050, 2), (1048576, 0)]          # two inside a row's curve, one between two rows
    assert p["range"]["edges"] == [(1 << 20, 0)]
    assert p["point"]["level_rounds"] == 128 and p["range"]["level_rounds"] == 128
    assert st.curves_launches(p, G, probs=3, c=c) == 1 + 4 * 2 + 1 + 2 * 2 == 14
    # fewer outputs, fewer launches: the count follows what is asked for
    assert st.curves_launches(p, G, outputs=("mean",), c=c) == 1 + 4 and st.curves_launches(p, G, outputs=("p_max",), c=c) == 2
    assert st.curves_launches(p, G, outputs=("quantiles", "range_quantiles"), probs=1, c=c) == 1 + 4 + 1 + 2


def test_small_curves_shape_has_two_pieces_and_no_second_trip(c):
    n, G = st.small_rows(c), st.G_SMALL
    p = st.plan(n, st.S, G, 0, st.default_scratch("curves", c), c)
    assert (p["C"], p["chunks"], p["tiles"], p["workgroups"], p["trips_first"]) == (n, 1, 205, 205, 1)
    assert p["C"] * G == 1048900 and p["point"]["pieces"] == 2 and p["point"]["edges"] == [(209715, 1)] and p["range"]["pieces"] == 1
    assert st.curves_launches(p, G, probs=3, c=c) == 1 + 2 * 2 + 1 + 2 == 8
    q = st.plan(n, st.S, G, 8 * st.S * G * (1 << 16), st.default_scratch("curves", c), c)
    assert (q["C"], q["chunks"], q["last_chunk_rows"], q["point"]["pieces"]) == (1 << 16, 4, 13172, 1) and st.curves_launches(q, G, probs=3, c=c) == 24


def test_the_plan_restates_the_chunk_rule_of_the_cases_the_other_tests_assert(c):
    """The shapes whose rows per chunk, chunks and launches the existing GPU tests assert from the device's info: the same numbers from plan()."""
    p = st.plan(200000, 8, 1, 1 << 20, c=c)
    assert (p["C"], p["chunks"], p["tiles"], p["trips_first"]) == (16384, 13, 16, 1)
    p = st.plan(2 * 1024 + 1, 18, 1, 8 * 18 * 1088 + 8 * 18 * 63, c=c)
    assert (p["C"], p["chunks"], p["last_chunk_rows"], st.quantiles_launches(p)) == (1088, 2, 961, 4)
    for rows, S, G, scratch in ((200, 3, 3, 8 * 64 * 9), (200, 3, 3, 1), (10 ** 6, 400, 20, 0), (50, 3, 3, 0)):
        assert st.plan(rows, S, G, scratch, st.default_scratch("curves", c), c)["C"] == cv.chunk_rows(rows, S, G, scratch)


def test_the_grid_stride_of_k_level_fold_is_out_of_reach(c):
    """k_level_fold runs a thread per (level over a slab edge, draw) of ONE chunk and strides past GRID_MAX workgroups of BLOCK.  A slab edge has at
    most one level over it and a chunk holds at most scratch / (8 S) rows, so there are at most scratch / (8 x 64) such threads whatever S is: with
    the default scratch, which a call cannot raise, a quarter of one grid.  No shape reaches the second round; no test is owed for it."""
    most = st.default_scratch("groups", c) // (8 * st.SLAB)
    assert most == 131072 and most < c["GRID_MAX"] * c["BLOCK"] == 524288


def test_selection_covers_the_piece_edges_and_the_strided_tile(c):
    N = st.big_rows(c)
    sel = st.selection(N, st.G_BIG, c)
    for row in (0, 63, 349525 - 32, 349525, 349525 + 32, 699050 - 32, 699050 + 32, (1 << 20) - 64, (1 << 20) - 1, 1 << 20, N - 1):
        assert row in sel, row
    assert len(sel) == 64 + 65 + 65 + 129 and np.all(np.diff(sel) > 0)
    small = st.selection(st.small_rows(c), st.G_SMALL, c)
    assert 209715 - 32 in small and 209715 + 32 in small and st.small_rows(c) - 1 in small and len(small) == 64 + 65 + 64 - 32


@pytest.fixture(scope="module")
def chain(emul_lib):
    ch = st.make_chain(emul_lib, "emu_", st.big_rows())
    yield ch
    ch.close()


@pytest.mark.parametrize("shape,anchor", [("big", None), ("big", 0), ("small", None), ("small", 0)])
def test_ambiguity_share_of_the_rows_that_meet_the_model(chain, shape, anchor):
    rows, G = (st.big_rows(), st.G_BIG) if shape == "big" else (st.small_rows(), st.G_SMALL)
    sel = st.selection(rows, G)
    inp = st.curve_inputs(chain, rows, G, anchor, M=0 if anchor is not None else 1, offset=anchor is None)
    assert sum(int(chain.hit(s, inp["vars"]).sum()) for s in st.POOL) > 0
    ref, bd, extra = st.curve_model(chain, inp, sel, probs=())
    share = cv.ambiguity(ref, bd, extra)
    print(f"{shape}, anchor {anchor}: {share:.4f} of the (row, draw) pairs of the {len(sel)} selected rows are ambiguous")
    assert share <= cv.AMBIGUOUS_MAX, f"{share:.3f} of the (row, draw) pairs have no certain maximum or minimum: another GRID_SEED"
