"""The exact probit latents ALONE on chosen streams, where no GPU is needed (cases, model and tools: tests/latent_cases.py; the kernel itself:
tests/test_gpu_latents_exact.py).  The serial model is pinned to the oracle on every case, the emulated device layer to the oracle through the
latents-only entry (s4b_test_draw_latents), every case's claim about what it hits is asserted on the model's counts — a change of L_NB, L_CH or of
the lists cannot quietly stop a case from reaching its arm —, and the integer arithmetic of k_latents2's refill / no-progress guard is walked on the
host."""
import os
import re

import numpy as np
import pytest

import latent_cases as L
from conftest import ROOT, StateView, make_sampler

CASES = L.cases()
BY_NAME = {c.name: c for c in CASES}


def _two_draws(lib, prefix, case):
    """The case injected into a fresh sampler of `lib`, then two consecutive latents-only draws: the StateViews before, after one and after two."""
    s = make_sampler(lib, prefix, L.sampler_args(case))
    try:
        before = L.inject(s, case, StateView)
        s.test_draw_latents()
        one = StateView(s.get_state())
        s.test_draw_latents()
        two = StateView(s.get_state())
    finally:
        s.free()
    return before, one, two


def _rng_words(sv):
    return sv.get("r_rng")[:625]


def test_untempering_and_the_backward_generator_round_trip():
    g = np.random.default_rng(0)
    w = np.concatenate([g.integers(0, 1 << 32, size=4096, dtype=np.uint64).astype(np.uint32), np.array([0, 1, 0x80000000, 0xFFFFFFFF], dtype=np.uint32)])
    assert np.array_equal(L.temper(L.untemper(w)), w) and np.array_equal(L.untemper(L.temper(w)), w)
    blk = g.integers(0, 1 << 32, size=624, dtype=np.uint64).astype(np.uint32)
    nxt = L.mt_forward(blk)
    raw, end = L.raw_stream(np.concatenate([[np.uint32(624)], blk]).astype(np.uint32), 624)
    assert np.array_equal(L.temper(nxt), raw) and np.array_equal(end[1:], nxt) and end[0] == 624      # (lazy: the 624th output leaves mti = 624)
    back = L.mt_backward(nxt)
    assert np.array_equal(back[1:], blk[1:]) and (back[0] ^ blk[0]) & 0x80000000 == 0
    six = nxt
    for _ in range(5):
        six = L.mt_forward(six)
    b = six
    for _ in range(6):
        b = L.mt_backward(b)
    f = b
    for _ in range(6):
        f = L.mt_forward(f)
    assert np.array_equal(f, six)
    # 623 words of a block are free, the last follows (one bit of choice)
    free = g.integers(0, 1 << 32, size=624, dtype=np.uint64).astype(np.uint32)
    for bit in (0, 1):
        free[623] = L.last_word(free, bit)
        assert np.array_equal(L.mt_forward(L.mt_backward(free)), free)


def test_every_case_is_inside_the_domain_and_away_from_ties():
    for c in CASES + L.cases(big=True)[-1:]:
        for m in (c.m1, c.m2):
            assert m["used"].max() <= L.MAX_POSITIONS, c.name
            assert m["margin"].min() >= L.MIN_MARGIN, (c.name, m["margin"].min())
            if not c.claim.get("exact_q"):
                assert m["qmargin"].min() >= L.MIN_MARGIN, (c.name, m["qmargin"].min())
            L.table_walk(m["used"], L.kernel_limits())           # (asserts: no observation is refused from slack 0)


def test_the_size_list_covers_the_edges_the_kernel_has():
    lim = L.kernel_limits()
    nb, ch = lim["nb"], lim["ch"]
    need = {nb - 1, nb, nb + 1, 63, 64, 65, ch - 1, ch, ch + 1, 2 * ch, 2 * ch + 1}
    assert need <= set(L.SIZES) and min(L.SIZES) < 8
    names = [c.name for c in CASES if c.name.startswith("size-")]
    for kind in ("normal", "wide"):
        for mti in L.START_MTI:
            assert any(f"-{kind}-mti{mti}" in n for n in names), (kind, mti)
        for n in L.SIZES:
            assert any(x.startswith(f"size-n{n}-{kind}-") for x in names)
    # a norm_rand() that straddles two generator blocks (position 623 of a block is its first uniform), with either parity of the start
    hits = sum(int(((m["start"] % 624 == 623) & ~m["exp"]).sum()) for c in CASES for m in (c.m1, c.m2))
    assert hits >= 8, hits
    wide = [c for c in CASES if "-wide-" in c.name and c.n >= 2047]
    assert all(c.m1["exp"].sum() > c.n // 4 and (np.abs(c.fits + c.offset) > 7.0).any() for c in wide)


def test_block_boundary_cases_end_on_a_block_boundary():
    cs = [c for c in CASES if c.name.startswith("boundary-")]
    lim = L.kernel_limits()
    assert len(cs) >= 3 and any(c.n > lim["ch"] for c in cs)
    for c in cs:
        total = int(c.rng[0]) + int(c.m1["used"].sum())
        assert total % 624 == 0 and total >= 624 and c.m1["end"][0] == 624, c.name
        # lazy regeneration: the state handed back is the block the last position came from, not the next one
        blocks = total // 624 - 1
        mt = c.rng[1:]
        for _ in range(blocks):
            mt = L.mt_forward(mt)
        assert np.array_equal(c.m1["end"][1:], mt), c.name


def test_crafted_runs_hit_what_they_claim():
    lim = L.kernel_limits()
    nb, ch = lim["nb"], lim["ch"]
    seen_next, seen_idx, sentinels = set(), set(), 0
    for c in CASES:
        if not c.name.startswith("run-"):
            continue
        k, m = c.claim["obs"], c.m1
        assert m["norm_rej"][k] == c.claim["rejections"] and m["used"][k] == c.claim["used"] and m["start"][k] == c.claim["start"], c.name
        assert m["start"][k] + m["used"][k] - 1 - int(c.rng[0]) <= 4366 and not m["exp"][k]
        others = np.delete(np.arange(c.n), [k, k - 1] if c.claim["front"] else [k])
        assert (m["used"][others] == 2).all(), c.name
        if c.claim["front"]:
            assert m["exp"][k - 1] and m["used"][k - 1] == 5 and m["exp_len"][k - 1] == 4 and m["start"][k] % 2 != (int(c.rng[0]) % 2), c.name
        idx, slack, nxt, sent = L.table_walk(m["used"], lim)
        sentinels += sent
        seen_next.add(int(nxt[k])); seen_idx.add((c.claim["rejections"], int(idx[k])))
        if c.name.startswith("run-sentinel"):
            assert sent == 1 and idx[k] == 0 and slack[k] == 0 and nxt[k] == c.claim["used"] - 2, c.name      # refused at slack 3, opens the next batch
        elif c.name.startswith("run-chunk"):
            assert k in (ch - 1, ch) and idx[k] == (nb - 1 if k == ch - 1 else 0) and m["start"][k] // 624 == 6, c.name
        else:
            assert sent == 0 and nxt[k] == slack[k] + c.claim["used"] - 2, c.name
    # either side of the two ballots (32 candidates of one parity), of the chain's stop at 64, the last representable entries, the sentinel
    assert {62, 63, 64, 65, 66, 252, 254} <= seen_next, sorted(seen_next)
    assert sentinels == 2
    for r in (31, 32, 33, 126, 127):
        assert {(r, 0), (r, nb // 2), (r, nb - 1)} <= seen_idx, (r, sorted(seen_idx))
    assert max(c.max_used() for c in CASES) == L.MAX_POSITIONS


def test_crafted_exponential_cases_hit_what_they_claim():
    lim = L.kernel_limits()
    for c in CASES:
        if not c.name.startswith("exp-"):
            continue
        m, cl = c.m1, c.claim
        if "exp_obs" in cl:
            assert m["exp"][cl["exp_obs"]].all() and not m["exp"][len(cl["exp_obs"]):].any(), c.name
            if "aa" in cl:
                assert (m["aa"][cl["exp_obs"]] == cl["aa"]).all()
                assert np.signbit(c.fits[2:4] + c.offset[2:4]).all() and not np.signbit(c.fits[:2] + c.offset[:2]).any()
            if "lowers" in cl:
                assert np.allclose(m["aa"][cl["exp_obs"]], [0.5 * (v + np.sqrt(v * v + 4.0)) for v in cl["lowers"]], rtol=1e-15)
            continue
        k = cl["obs"]
        assert m["exp"][k] and m["start"][k] == cl["start"], c.name
        for key in ("exp_len", "exp_rej", "used"):
            if key in cl:
                assert m[key][k] == cl[key], (c.name, key, m[key][k])
        if "crosses" in cl:
            assert m["start"][k] < cl["crosses"] < m["start"][k] + 17
        if "range_end" in cl:      # the first refill generates whole blocks until 1536 positions lie ahead: three of them from a small mti
            assert 3 * 624 - int(c.rng[0]) >= 1536 > 2 * 624 - int(c.rng[0])
            assert m["start"][k] + 17 > cl["range_end"] and m["start"][k] - cl["range_end"] in (-10, 1)
    assert lim["emax"] >= 17 + 1        # the longest exp_rand() plus the uniform after it must fit behind the last E / EL entry
    # 17 is the longest exp_rand() there is: the search ends at q[15] = 1.0 at the latest, and only v = 1.0 (output 0x80000000) gets there
    assert L._exp_rand([0.5] + [0.3] * 20, 0)[1] == 17 and max(int(m["exp_len"].max()) for c in CASES for m in (c.m1, c.m2)) == 17


def test_the_conventions_case_does_not_cancel():
    c = BY_NAME["conventions-offset-1e3"]
    mean = c.fits + c.offset
    assert np.abs(c.offset).max() > 1e3 and np.abs(mean).max() < 8.0
    assert np.abs(c.lat - c.fits).min() > 1e-3 and np.abs(c.m1["lat"] + c.offset - mean).max() < 10.0


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_model_and_emulated_layer_match_the_oracle(oracle_lib, emul_lib, case):
    """Two consecutive draws.  Model == oracle: generator words and mti bit for bit, latents to 1e-12 relative (same libm).  Emulated layer == oracle:
    generator and latents bit for bit in the first draw (the inputs lie on a grid where latent - (latent - fits) is exact); the second starts from
    latents off that grid, where the emulated layer's mean = (latent - residual) + offset carries a rounding the oracle's fits + offset has not."""
    b0, o1, o2 = _two_draws(oracle_lib, "orc_", case)
    _, e1, e2 = _two_draws(emul_lib, "emu_", case)
    assert np.array_equal(_rng_words(b0), case.rng) and np.array_equal(b0.get("latents"), case.lat)
    for m, o, e, first in ((case.m1, o1, e1, True), (case.m2, o2, e2, False)):
        assert np.array_equal(_rng_words(o), m["end"]), case.name
        np.testing.assert_allclose(o.get("latents"), m["lat"], rtol=1e-12, atol=0.0)
        assert np.array_equal(_rng_words(e), _rng_words(o)), case.name
        if first:
            assert np.array_equal(e.get("latents"), o.get("latents")), case.name
        else:
            np.testing.assert_allclose(e.get("latents"), o.get("latents"), rtol=1e-6, atol=1e-9)
        for k in ("offset", "win", "ecuyer", "q", "scale"):
            assert np.array_equal(o.get(k), b0.get(k)) and np.array_equal(e.get(k), b0.get(k)), k
        assert np.array_equal(o.get("total_fits"), case.fits)
        np.testing.assert_allclose(e.get("total_fits"), case.fits, rtol=1e-6, atol=1e-9)
        for (na, ma), (nb, mb) in zip(o.trees, b0.trees):
            assert np.array_equal(na, nb) and np.array_equal(ma, mb)


def test_the_entry_is_refused_where_it_does_not_apply(oracle_lib, emul_lib):
    from conftest import friedman_case
    args, _ = friedman_case(n=60, T=3, warmup=2, iter=4)
    for lib, pfx in ((emul_lib, "emu_"), (oracle_lib, "orc_")):
        s = make_sampler(lib, pfx, args)
        try:
            with pytest.raises(RuntimeError, match="test_draw_latents"):
                s.test_draw_latents()
        finally:
            s.free()


def test_one_step_beyond_the_domain_is_known_and_stays_off_the_cases(oracle_lib, emul_lib):
    """128 rejected normals: the serial implementations go on (and agree), the model of the table says the kernel must refuse — the divergence
    DESIGN.md 7 records.  The case is not in cases(): nothing of the suite sends it to a GPU."""
    c = L.over_limit_case()
    assert c.m1["used"][0] == 258 and c.m1["norm_rej"][0] == 128 and c.m1["margin"].min() >= L.MIN_MARGIN
    assert c.name not in {x.name for x in L.cases(big=True)}
    with pytest.raises(AssertionError, match="outside the kernel's domain"):
        L.table_walk(c.m1["used"], L.kernel_limits())
    _, o1, _ = _two_draws(oracle_lib, "orc_", c)
    _, e1, _ = _two_draws(emul_lib, "emu_", c)
    assert np.array_equal(_rng_words(o1), c.m1["end"]) and np.array_equal(_rng_words(e1), c.m1["end"])
    assert np.array_equal(o1.get("latents"), e1.get("latents"))


def test_refill_keeps_the_table_fed_and_the_guard_reachable():
    """k_latents2's integer bookkeeping on the host.  base = position of the next draw, nblk = blocks generated (positions below 624 nblk exist).

    (a) The refill condition, restated from the source, leaves at least 1536 and fewer than 2160 positions ahead of base from every reachable state, so
        the ring (L_RING) is never lapped and the block of the hand-back is still among the L_BLK kept ones.
    (b) What one batch reads lies inside what refill left: at most 2 (L_NB - 1) + 63 positions of start, two ballots of 64, and an observation inside
        the domain (256 positions) — so inside the domain `bad` is never set, and a batch that resolves NOTHING means its first observation is
        outside the domain.  The guard must therefore stop on cnt == 0 alone; the condition it had before (ring full: more than 3472 ahead) contradicts
        (a) and could never hold, which left a one-workgroup kernel repeating the same batch for ever."""
    src = open(os.path.join(ROOT, "stan4bart_amd", "csrc", "dev_hip.hip")).read()
    lim = L.kernel_limits()
    assert "while ((long long)624 * nblk - base < 1536) {" in src
    assert "shStop = cnt == 0 ? 1 : 0;" in src
    assert "624 * (nblk + 1) - base > L_RING" not in src
    body = src[src.index("void k_latents2("):src.index("void k_latents_finish(")]
    assert len(re.findall(r"shStop = ", body)) == 1

    def refill(base, nblk):
        while 624 * nblk - base < 1536:
            nblk += 1
        return nblk
    worst_ahead, worst_behind = 0, 0
    for mti in range(0, 625):
        base, nblk = mti, 1
        # every advance a batch can make: 2 per resolved observation plus a last slack of at most 254; walk the extremes and a spread between them
        for step in (2, 64, 2 * lim["nb"] + 63, 2 * (lim["nb"] - 1) + 254 + 2):
            b, k = base, nblk
            for _ in range(200):
                k = refill(b, k)
                ahead = 624 * k - b
                assert 1536 <= ahead < 1536 + 624
                worst_ahead = max(worst_ahead, ahead)
                reach = 2 * (lim["nb"] - 1) + 63 + L.MAX_POSITIONS + lim["emax"] + 128
                assert reach < 1536 - lim["emax"] - 1
                # the block the hand-back reads (that of position b, or the one before on a boundary) is within the last L_BLK generated
                hb = b // 624 - (1 if b % 624 == 0 and b > 0 else 0)
                worst_behind = max(worst_behind, k - 1 - hb)
                b += step
    assert worst_ahead + 2 * (lim["nb"] - 1) + 254 + 2 < lim["ring"] and worst_behind < lim["blk"]
