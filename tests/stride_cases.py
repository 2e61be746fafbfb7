"""Which loops of the chunked read-outs a call shape reaches (stan4bart_amd/csrc/dev_quantile.inc: chunk_plan, chunk_grid; dev_groups.inc:
LevelsSummary, k_level_rows; dev_contrast.inc, readout_curves.inc: the launches of a chunk) — restated in plain Python over the constants READ from the
sources, and the shapes, the chain and the inputs shared by tests/test_readout_strides.py (CPU) and tests/test_gpu_readout_strides.py (GPU).

Three loops of these read-outs go round more than once only past a compile-time threshold, which no other test reaches:
  the tile loop of the value kernels   for (tile = blockIdx.x; tile < tiles; tile += gridDim.x) in k_predict_values, k_contrast_values, k_curve_values:
                                       a second trip of a workgroup past PS_GRID_MAX tiles of PS_BLOCK rows in ONE chunk;
  the pieces of LevelsSummary::run     more than GP_SORT_LEVELS rows of a [levels x draws] matrix: offsets first + l0 of the outputs, l0 S of the values;
  the grid stride of k_level_rows      more than GRID_MAX workgroups of BLOCK / 64 levels in one launch.
plan() says for a shape how often each goes round; the CPU test holds the shapes below to exactly the coverage they are there for, so that a changed
constant fails there instead of silently taking the GPU tests off their loops."""
import os
import re

import numpy as np

import curve_cases as cv
import readout_cases as rc
import summary_cases as sc

CSRC = os.path.join(rc.ROOT, "stan4bart_amd", "csrc")
SLAB = 64          # GP_SLAB, CV_SLAB, CT_SLAB: rows per slab of the reductions over the rows, part of the interface


def _code(name):
    with open(os.path.join(CSRC, name)) as f:
        return "\n".join(line.split("//")[0] for line in f.read().splitlines())


def constants():
    """The constants that decide the loops, read from the sources; the statements restated below are asserted to still be there."""
    summary, readout, quantile, groups = _code("dev_summary.inc"), _code("dev_readout.inc"), _code("dev_quantile.inc"), _code("dev_groups.inc")
    hip, curves, contrast = _code("dev_hip.hip"), _code("readout_curves.inc"), _code("dev_contrast.inc")

    def const(src, name, kind="int"):
        return int(re.search(r"constexpr " + kind + " " + name + r" = (\d+);", src).group(1))
    c = dict(PS_BLOCK=const(summary, "PS_BLOCK"), PS_GRID_MAX=const(readout, "PS_GRID_MAX"), GRID_MAX=const(hip, "GRID_MAX"), BLOCK=const(hip, "BLOCK"),
             QT_SORT=const(quantile, "QT_SORT"))
    c["GP_SORT_LEVELS"] = 1 << int(re.search(r"constexpr int64_t GP_SORT_LEVELS = 1 << (\d+);", groups).group(1))
    c["S4B_QT_SCRATCH_MIB"] = int(re.search(r"#define S4B_QT_SCRATCH_MIB (\d+)", quantile).group(1))
    c["CV_SCRATCH_DEFAULT"] = int(re.search(r"constexpr int64_t CV_SCRATCH_DEFAULT = \(int64_t\)(\d+) << 20;", curves).group(1)) << 20
    assert "constexpr int64_t QT_SCRATCH_DEFAULT = (int64_t)S4B_QT_SCRATCH_MIB << 20;" in quantile
    for name, src in (("GP_SLAB", groups), ("CV_SLAB", curves), ("CT_SLAB", contrast)):
        assert const(src, name) == SLAB, name
    # the chunk rule, the grid of a value launch and the three loops
    assert "scratch / (8 * S * perRowDraw) / multiple * multiple" in quantile and "p.R = std::max(1, QT_SORT / p.Sp);" in quantile
    assert "std::min<int64_t>((a.chunkRows + PS_BLOCK - 1) / PS_BLOCK, PS_GRID_MAX)" in quantile
    loop = "for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x)"
    assert loop in quantile and loop in contrast and loop in curves
    assert "for (int64_t l0 = 0; l0 < n; l0 += GP_SORT_LEVELS)" in groups
    assert "l < a.L; l += (int64_t)gridDim.x * (BLOCK / 64)" in groups
    assert groups.count("std::min<int64_t>(GRID_MAX, (L + BLOCK / 64 - 1) / (BLOCK / 64))") == 1
    assert "std::min<int64_t>(GRID_MAX, (c.L + BLOCK / 64 - 1) / (BLOCK / 64))" in groups
    # the launches of a chunk of curves_run, restated by curves_launches()
    for said in ("chunk_plan(r.nT, r.S, c.scratchBytes, CV_SCRATCH_DEFAULT, c.G, 64)",
                 "const bool perPoint = c.mean || c.m2 || Q, extremes = c.pMax || c.pMin || c.rangeMean || c.rangeM2 || c.rangeQuantiles;",
                 "if (perPoint) sum.run(stream, launched, a.vals, a.chunkRows * c.G, a.chunk0 * c.G, mean, m2, quantiles, r.nT * c.G);",
                 "if (rangeMean || rangeM2 || rangeQuantiles) sum.run(stream, launched, a.base, a.chunkRows, a.chunk0, rangeMean, rangeM2, rangeQuantiles, r.nT);"):
        assert said in curves, said
    for said in ("chunk_plan(r.nT, r.S, ar.scratchBytes, QT_SCRATCH_DEFAULT, 1, 64)", "if (Q) sum.run(stream, launched, g.lev, c.L, 0, nullptr, nullptr, quantiles, c.L);"):
        assert said in groups, said
    return c


def _ceil(a, b):
    return -(-a // b)


def default_scratch(readout, c=None):
    c = c or constants()
    return c["CV_SCRATCH_DEFAULT"] if readout == "curves" else c["S4B_QT_SCRATCH_MIB"] << 20


def pieces(n, G=1, c=None):
    """LevelsSummary::run over n rows of a matrix whose row x is (x // G, x % G): the number of pieces, the (row, grid point) every piece after the
    first begins at, and the rounds of k_level_rows' grid-stride loop in the largest piece."""
    c = c or constants()
    piece = c["GP_SORT_LEVELS"]
    per_round = c["GRID_MAX"] * (c["BLOCK"] // 64)
    return dict(pieces=_ceil(n, piece), edges=[(l0 // G, l0 % G) for l0 in range(piece, n, piece)], level_rounds=_ceil(min(piece, n), per_round))


def plan(rows, S, G=1, scratch_bytes=0, default=None, c=None):
    """chunk_plan and chunk_grid restated for `rows` rows, S pooled draws, G values per row and draw: rows per chunk, chunks, and of the FIRST chunk
    (every chunk but the last is like it) the tiles, the workgroups along the rows, the trips of workgroup 0 and of the last workgroup through the tile
    loop, the rows of the last tile, the slabs, and LevelsSummary's pieces over its C G per-point rows and over its C range rows."""
    c = c or constants()
    default = default_scratch("quantiles", c) if default is None else default
    scratch = min(scratch_bytes, default) if scratch_bytes > 0 else default
    C = min(rows, max(64, scratch // (8 * S * G) // 64 * 64))
    chunks = _ceil(rows, C)
    tiles = _ceil(C, c["PS_BLOCK"])
    wg = min(tiles, c["PS_GRID_MAX"])
    Sp = 1 << max(0, (S - 1).bit_length())
    return dict(C=C, chunks=chunks, last_chunk_rows=rows - (chunks - 1) * C, tiles=tiles, workgroups=wg, trips_first=_ceil(tiles, wg),
                trips_last=(tiles - wg) // wg + 1, last_tile_rows=C - (tiles - 1) * c["PS_BLOCK"], slabs=_ceil(C, SLAB), Sp=Sp, R=max(1, c["QT_SORT"] // Sp),
                point=pieces(C * G, G, c), range=pieces(C, 1, c))


def _chunk_rows(p):
    return [p["C"]] * (p["chunks"] - 1) + [p["last_chunk_rows"]]


def quantiles_launches(p):
    """quantile_run: the value kernel and the sort per chunk."""
    return 2 * p["chunks"]


def contrast_launches(p, per_row=True, weights=0, probs=0):
    """contrast_run: per chunk the value kernel, the reduce (per-row outputs or weights), the fold (weights), the sort (probs)."""
    return p["chunks"] * (1 + (1 if per_row or weights else 0) + (1 if weights else 0) + (1 if probs else 0))


def groups_launches(p, L, probs=0, fold_chunks=0, c=None):
    """groups_run: per chunk the value kernel and the reduce, the fold in `fold_chunks` chunks (those with a level over a slab edge), then k_level_rows
    once over all L levels and the sort in pieces of the level matrix."""
    return 2 * p["chunks"] + fold_chunks + 1 + (pieces(L, 1, c)["pieces"] if probs else 0)


def curves_launches(p, G, outputs=None, probs=0, c=None):
    """curves_run: per chunk the value kernel; for the per-point outputs a k_level_rows (mean or m2) and a sort (probs) per piece of its C G rows; for
    the extremes k_curve_rows and, for the range outputs, a k_level_rows (range_mean or range_m2) and a sort (range_quantiles) per piece of its C rows."""
    from stan4bart_amd.abi import CURVES_OUTPUTS
    out = set(CURVES_OUTPUTS if outputs is None else outputs)
    Q = probs if "quantiles" in out else 0
    per_point = bool(out & {"mean", "m2"}) + bool(Q)
    ranges = bool(out & {"range_mean", "range_m2"}) + bool(Q and "range_quantiles" in out)
    extremes = bool(out & {"p_max", "p_min", "range_mean", "range_m2", "range_quantiles"})
    n = 0
    for rows in _chunk_rows(p):
        n += 1 + per_point * pieces(rows * G, G, c)["pieces"] + (1 + ranges * pieces(rows, 1, c)["pieces"] if extremes else 0)
    return n


# ---- the shapes ------------------------------------------------------------------------------------------------------------------------------------------
S = 3                        # pooled draws: the stored sampler of 2 draws takes the call, the one of 1 draw is its peer
POOL = (2, 1)
STEPS = (1, 1, 6)            # stored samplers of 1, 2 and 8 draws of readout_cases.PREDICT_CASES["cap-exact"]'s chain (n = 400, 5 trees, 8 kept draws)
PROBS = (0.0, 0.5, 1.0)      # h = p (S - 1) is an integer for each: the three quantiles of a row are its three values, sorted, bit for bit
CURVE_PROBS = (0.025, 0.5, 1.0)
G_BIG, G_SMALL = 3, 5
GRID_SEED = 0                # of curve_cases.grid_of; the CPU test holds the ambiguity share of the rows that meet the model under curve_cases.AMBIGUOUS_MAX
MARGIN = 32                  # rows on either side of a piece-edge row that meet the model


def big_rows(c=None):
    """One tile of 65 rows more than one grid of tiles: a full wave and a wave with one live lane in the second trip of workgroup 0."""
    c = c or constants()
    return c["PS_GRID_MAX"] * c["PS_BLOCK"] + 65


def small_rows(c=None):
    """65 rows past the row whose G_SMALL-point curve the first piece of LevelsSummary ends in: two pieces, far below one grid of tiles."""
    c = c or constants()
    return c["GP_SORT_LEVELS"] // G_SMALL + 65


def compare_scratch(G=1):
    """scratch_bytes of the comparison calls: chunks of 2^18 rows."""
    return 8 * S * G * (1 << 18)


def selection(rows, G, c=None):
    """The rows of a curves shape that meet the model: the first 64, MARGIN on either side of every piece-edge row, and from 64 rows in front of the
    last full grid of tiles (the end of the last single-trip tile) to the end (where the shape has one: the whole strided tile)."""
    c = c or constants()
    pick = [np.arange(min(64, rows))]
    for row, _ in pieces(rows * G, G, c)["edges"]:
        pick.append(np.arange(max(0, row - MARGIN), min(rows, row + MARGIN + 1)))
    cap = c["PS_GRID_MAX"] * c["PS_BLOCK"]
    pick.append(np.arange(cap - 64, rows) if rows > cap else np.arange(max(0, rows - 64), rows))
    return np.unique(np.concatenate(pick))


# ---- the chain and the inputs ------------------------------------------------------------------------------------------------------------------------------
def make_chain(lib, prefix, rows):
    """test_gpu_predict_contrast.Chain over the cap-exact chain: the hard rows of its rules in front, new rows behind them, `rows` in all."""
    from test_gpu_predict_contrast import Chain
    args = rc.PREDICT_CASES["cap-exact"][0]()
    assert args.n_trees == 5 and args.iter - args.warmup == sum(STEPS)
    chain = Chain(lib, args, steps=STEPS, rows=rows, prefix=prefix)
    assert len(chain.x) == rows and chain.n_hard < 64 * 1024
    return chain


def curve_inputs(chain, rows, G, anchor, M=0, offset=False, seed=GRID_SEED):
    """curve_cases.inputs for these shapes: the busiest predictor of the pool, G grid points, per pooled sampler a dense table of its own."""
    hits = [sum(int(chain.hit(s, v).sum()) for s in POOL) for v in range(chain.P)]
    vs = [int(np.argmax(hits))]
    grid = cv.grid_of(chain, vs, G, seed=seed)
    tables = [sc.linear_parts(rows, s, M, 0, seed=seed + 31 * j) for j, s in enumerate(POOL)]
    off = 10.0 * float(chain.range[1] - chain.range[0]) * np.random.default_rng(seed).uniform(-1.0, 1.0, rows) if offset else None
    linear = dict(offset=off, dense=tables[0].get("dense"))
    call = dict(linear, dense_coef=tables[0].get("dense_coef"), link=0, anchor=anchor, peers=[chain.stored[s] for s in POOL[1:]],
                peer_dense_coef=[t["dense_coef"] for t in tables[1:]] if M else None)
    parts = [dict(predict_bart=chain.stored[s].predict_bart, trees=chain.trees[s], hit=chain.hit(s, vs), dense_coef=t.get("dense_coef")) for s, t in zip(POOL, tables)]
    return dict(x=np.asfortranarray(chain.x[:rows]), vars=vs, grid=grid, anchor=anchor, call=call, parts=parts, linear=linear)


def curve_model(chain, inp, sel, probs=CURVE_PROBS):
    """curve_cases.model on the rows `sel` of the call."""
    linear = {k: (None if v is None else v[sel]) for k, v in inp["linear"].items()}
    return cv.model(inp["parts"], inp["x"][sel], inp["vars"], inp["grid"], chain.T, chain.range, chain.binary, anchor=inp["anchor"], link=0, probs=probs, **linear)
