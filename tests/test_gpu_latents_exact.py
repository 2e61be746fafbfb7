"""k_latents2 + k_latents_finish ALONE on the MI355X, on chosen streams (cases, serial model and tools: tests/latent_cases.py; their CPU checks:
tests/test_latents_exact.py).  For every case the same state blob is injected into an oracle sampler and a HIP sampler, the latents-only entry
(s4b_test_draw_latents) is called once on each and the states are compared: R's generator — 624 words and mti — bit for bit, the latents and every
untouched field at the project's bar (rtol 1e-6, atol 1e-9).  Then a second draw from the state the first left: the generator state the kernel
hands back is what the next draw starts from.

What the cases select in the kernel (dev_hip.hip; each claim is asserted on the model in the CPU file): the plain loop after the two ballots (32 and
more rejections from one start), next-slacks either side of 64, the last representable ones (252, 254) and the sentinel, the 17-position exp_rand(),
exp_rand() across a block end and across the end of the first generated range, lower = +-0.0 / 8 / 40, start positions 1, 2, 623, 624, draws that
end on a block boundary, batch, wave and chunk edges of n, the chunk edge six blocks in, offsets of 1e3 under means of order 1.

No case leaves the kernel's domain (at most 256 positions per observation: the builder asserts it); a stream beyond it is not run here."""
import numpy as np
import pytest

import latent_cases as L
from conftest import StateView, assert_state_parity, make_sampler

pytestmark = pytest.mark.gpu

CASES = L.cases(big=True)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_kernel_matches_the_oracle_on_a_chosen_stream(oracle_lib, hip_lib, case):
    args = L.sampler_args(case)
    so, sh = make_sampler(oracle_lib, "orc_", args), make_sampler(hip_lib, "s4b_", args)
    try:
        assert sh.get_latent_mode() == 0
        blob = L.inject(so, case, StateView).bytes()
        sh.set_state(blob)
        for m in (case.m1, case.m2):
            so.test_draw_latents()
            sh.test_draw_latents()
            a, b = StateView(so.get_state()), StateView(sh.get_state())
            ctx = f"{case.name}: " + ", ".join(f"{k} = {v}" for k, v in case.claim.items())
            assert np.array_equal(a.get("r_rng")[:625], m["end"]), ctx + " (oracle against the model)"
            assert b.get("r_rng")[0] == a.get("r_rng")[0], ctx + f": mti {b.get('r_rng')[0]} against {a.get('r_rng')[0]}"
            assert np.array_equal(a.get("r_rng"), b.get("r_rng")), ctx + ": generator words differ"
            d = np.abs(a.get("latents") - b.get("latents"))
            bad = np.nonzero(d > 1e-9 + 1e-6 * np.abs(a.get("latents")))[0]
            assert bad.size == 0, ctx + f": {bad.size} latents differ, first at observation {bad[0]} ({b.get('latents')[bad[0]]!r} against {a.get('latents')[bad[0]]!r})"
            assert_state_parity(a, b)
            assert np.array_equal(b.get("offset"), case.offset)
            np.testing.assert_allclose(b.get("total_fits"), case.fits, rtol=1e-6, atol=1e-9)
    finally:
        so.free(); sh.free()


def test_the_entry_is_refused_where_it_does_not_apply(hip_lib):
    """a continuous response has no latents.  (In latent mode 1 the entry runs k_latents_par and is checked value by value:
    tests/test_gpu_latents_par_alone.py.)"""
    from conftest import friedman_case
    s = make_sampler(hip_lib, "s4b_", friedman_case(n=60, T=3, warmup=2, iter=4)[0])
    try:
        with pytest.raises(RuntimeError, match="test_draw_latents"):
            s.test_draw_latents()
    finally:
        s.free()
