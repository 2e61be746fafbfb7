"""k_latents_par ALONE on the MI355X against the host model of tests/latent_par_cases.py (model, bounds, cases; their CPU checks:
tests/test_latents_par_alone.py).  For every case a mode-1 sampler is created, the case's state — offsets, fits, previous latents, Philox key and
draw index — is injected, the latents-only entry (s4b_test_draw_latents) is called and the state read back; then a second draw from the state the
first left, the model taking its means from that blob.  After each draw: every latent within 4 x its derived bound of the model's (the message names
the observation, its trip of the grid-stride loop, the attempt and the deviate), the truncation, total_fits unchanged, the key bit-identical, the draw
index exactly one further (also from 2^32 - 1 to 2^32), one more launch, and every other byte of the blob as it was (R's stream is not touched).

What the cases select (each claim asserted on the model in the CPU file): one to five trips of the grid-stride loop with a ragged last one, one / two /
65 / 257 / the capped 1 024 workgroups, observation words beyond 16 bits, draw indices 0, 1, 2^32 - 1 -> 2^32, 2^32, 2^63 + 5, keys with a zero low
half, a zero high half, all ones and the sampler's own, bounds +-0.0, -1e-300, +-8, +-40, 1e8, y mixed and all of one kind, offsets of 1e3 under means
of order 1; in every case of 256 observations or more both branches with two and with three and more attempts and the second Box-Muller deviate.

Also: the first 1 000 observations bit-equal at n = 1 000, 1 025 and 65 537 (a latent does not depend on the geometry); the key of a fresh sampler
against the Python hash; run() advances the draw index by `thin` per iteration; the one reported failure (a mean whose square overflows ends with the
error word S4B_ERR_I_LATENT — the kernel returns normally —, and the next sampler draws correctly)."""
import numpy as np
import pytest

import latent_par_cases as P
from conftest import StateView, make_sampler

pytestmark = pytest.mark.gpu

RATIOS = {}          # group of cases -> quantity -> largest observed ratio to its derived bound (reported, never asserted: the bounds are)


def _group(case):
    return "n = %d" % case.n if case.name.startswith("n") else case.name.split("-")[0]


def _note(case, what, value):
    g = RATIOS.setdefault(_group(case), {})
    g[what] = max(g.get(what, 0.0), float(value))


def _ratio(d, bound):
    return np.divide(d, bound, out=np.zeros_like(d), where=d > 0)


def _check_draw(case, m, fold, before, after, grid, block):
    """One draw: the state `after` against the model m of the draw from the state `before` (fold: the total_fits of `before`, the kernel's fOld)."""
    ctx = f"{case.name} (draw index {before.index:#x}, key {before.key:#018x})"
    assert int(m["undecided"].sum()) == 0, ctx + ": a decision of the model is closer to a tie than the bounds allow"
    lat, fits = after.sv.get("latents"), after.sv.get("total_fits")
    want, bound = P.latent_of(case.y, case.offset, fold, m, m["pert"])
    d = np.abs(lat.astype(P.LD) - want).astype(np.float64)
    assert np.all(np.isfinite(lat))
    r = _ratio(d, bound)
    i = int(np.argmax(r))
    _note(case, "latent", r[i])
    for br, name in ((0, "z0"), (1, "z1"), (2, "exponential")):
        if np.any(m["branch"] == br):
            _note(case, "latent, " + name, r[m["branch"] == br].max())
    assert r[i] <= P.BOUND_FACTOR, ctx + f": observation {i} (trip {i // (grid * block)} of {grid} workgroups, attempt {m['attempts'][i]}, deviate {('z0', 'z1', 'exponential')[m['branch'][i]]}, " \
        f"lower {m['lower'][i]!r}): latent {lat[i]!r} against {want[i]!r}, {r[i]:.3g} times the bound {bound[i]:.3g}; {int((r > P.BOUND_FACTOR).sum())} observations beyond it"
    slack = P.C_FITS * P.U * np.maximum(np.abs(lat), np.abs(fits))          # (the blob holds fl(latent - R), not R)
    R = lat - fits
    assert np.all(np.where(case.y > 0.0, R >= -m["mean"] - slack, R <= -m["mean"] + slack)), ctx + ": a latent is on the wrong side of its truncation point"
    tf = _ratio(np.abs(fits - fold), P.C_FITS * P.U * np.maximum(np.abs(lat), np.abs(fits)))
    _note(case, "total_fits", tf.max())
    assert tf.max() <= 1.0, ctx + f": total_fits moved at observation {int(np.argmax(tf))}"
    assert after.key == before.key, ctx + f": the key became {after.key:#018x}"
    assert after.index == before.index + 1, ctx + f": the draw index became {after.index:#x}"
    assert after.rest() == before.rest(), ctx + ": a field other than latents, total_fits and the draw index changed"


def _two_draws(hip_lib, case):
    """The case through a sampler: the latents after the first and after the second draw (everything else is asserted on the way)."""
    lim = P.kernel_geometry()
    grid = P.geometry(case.n, lim)[0]
    s = make_sampler(hip_lib, "s4b_", P.sampler_args(case))
    out = []
    try:
        assert s.get_latent_mode() == 1
        fresh = P.ParState(s.get_state(), StateView)
        assert fresh.index == 0, "the sweep inside create draws its latents exactly: no parallel draw yet"
        if case.key == P.OWN_KEY:
            assert fresh.key == P.sampler_key(), f"{fresh.key:#018x}"
        P.inject(s, case, StateView)
        before = P.ParState(s.get_state(), StateView)
        assert before.key == case.key_value() and before.index == case.index
        assert np.array_equal(before.sv.get("latents"), case.lat) and np.array_equal(before.sv.get("offset"), case.offset)
        for k in range(2):
            fold = before.sv.get("total_fits")
            if k == 0:
                assert np.array_equal(fold, case.f1)
                m = case.m1
            else:
                m = case.model(before.key, before.index, fold)          # the means of the second draw come from the blob after the first
            launches = s.get_counters()[2]
            s.test_draw_latents()
            assert s.get_counters()[2] == launches + 1, "the latent draw of mode 1 is one launch"
            after = P.ParState(s.get_state(), StateView)
            _check_draw(case, m, fold, before, after, grid, lim["block"])
            out.append(after.sv.get("latents"))
            before = after
    finally:
        s.free()
    return out


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_kernel_matches_the_model(hip_lib, name):
    _two_draws(hip_lib, P.case(name))


def test_a_latent_does_not_depend_on_the_geometry(hip_lib):
    """The same (key, draw index, mean, y) in the first 1 000 observations of n = 1 000 (one workgroup, four trips), 1 025 (two workgroups, three trips)
    and 65 537 (65 workgroups): bit-equal latents after both draws."""
    got = [_two_draws(hip_lib, P.case(name)) for name in P.TRIPLE]
    for other, name in zip(got[1:], P.TRIPLE[1:]):
        for k in range(2):
            diff = np.nonzero(other[k][:1000] != got[0][k])[0]
            assert diff.size == 0, f"{name}, draw {k}: {diff.size} of the first 1 000 latents differ from n = 1 000, first at observation {diff[0]}"


@pytest.mark.parametrize("seed", [12345, 999])
def test_key_of_a_fresh_sampler(hip_lib, seed):
    s = make_sampler(hip_lib, "s4b_", P.sampler_args(P.case("n255-key-low0-draw1-ones")), seed=seed)
    try:
        ps = P.ParState(s.get_state(), StateView)
        assert (ps.key, ps.index) == (P.sampler_key(seed), 0), f"{ps.key:#018x}"
    finally:
        s.free()


@pytest.mark.parametrize("thin", [1, 3])
def test_run_advances_the_draw_index_by_thin(hip_lib, thin):
    """One latent draw per sweep: an iteration of run() after an injected state advances the draw index by exactly `thin`, across 2^32 as well."""
    case = P.case("n257-key-ones-draw-2p32")
    s = make_sampler(hip_lib, "s4b_", P.sampler_args(case, thin=thin))
    try:
        ps = P.inject(s, case, StateView)
        ps.index = (1 << 32) - 2
        s.set_state(ps.bytes())
        s.run(1, True)
        after = P.ParState(s.get_state(), StateView)
        assert (after.key, after.index) == (ps.key, (1 << 32) - 2 + thin)
        s.run(2, True)
        assert P.ParState(s.get_state(), StateView).index == (1 << 32) - 2 + 3 * thin
    finally:
        s.free()


def test_a_mean_whose_square_overflows_is_reported(hip_lib):
    """y = 0 and mean 1e200 (finite: set_state accepts it): lam = inf, no proposal in 4 096 attempts, the kernel ends normally with the error word and the
    entry raises; the sampler can be freed and the next sampler of the process draws correctly."""
    y = np.array([0.0, 1.0, 0.0, 1.0])
    z = np.zeros(4)
    case = P.Case("failure-mean-1e200", y, z, z, z, 7, 0)          # (built inside the domain; the blob below leaves it)
    s = make_sampler(hip_lib, "s4b_", P.sampler_args(case))
    try:
        ps = P.inject(s, case, StateView)
        fits = np.zeros(4)
        fits[0] = P.failure_lower()
        ps.sv.set("total_fits", fits)
        s.set_state(ps.bytes())
        with pytest.raises(RuntimeError, match="parallel latents"):
            s.test_draw_latents()
    finally:
        s.free()
    _two_draws(hip_lib, P.case("n1-own-key-draw0"))


@pytest.fixture(scope="module", autouse=True)
def report_the_largest_ratios():
    """Not a check and not a test: when the module is through, prints (under -s) the largest observed ratio to each derived bound per group of cases."""
    yield
    for group in sorted(RATIOS):
        print(f"largest ratios, {group}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(RATIOS[group].items())))
