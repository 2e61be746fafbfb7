"""Host-side mirror of the reference's user surface around the hot path: ``stan4bart()`` (fit + package the draws,
reference R/stan4bart.R:299-455 ``package_samples``) and the generics ``extract`` / ``fitted`` / ``predict``
(reference R/generics.R:168-484, 486-508, 608-724).

There is no R in this image, so the formula / model-frame front end is replaced by explicit arrays (see ``fit.py``);
everything after that point — array layouts ``[.., iterations, chains]``, chain combination, how the components are put
together, the user-offset rules, the probit link, prediction from the kept trees — follows the R code.  Posterior
predictive noise (``type = "ppd"``) and random effects of unseen grouping levels are drawn with numpy's generator,
not R's stream: they are post-hoc draws outside the sampler.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, Optional, Sequence

import numpy as np

from .abi import (CURVES_OUTPUTS, DESCRIBE_HDI_MAX, DESCRIBE_THRESHOLDS_MAX, GROUPS_LEVEL_BYTES_MAX, GROUPS_STATISTICS, PD_GRID_MAX, PROJECTION_COLUMNS_MAX,
                  SORTED_CUTS_MAX, SORTED_PROBS_MAX, SPREAD_THRESHOLDS_MAX, Sampler, ceil_fraction, fraction_count)
from .fit import GroupTerm, chain_seeds, hip_sampler_factory, make_sampler_args, make_z_csr, qr_back_transform
from .rcompat import RRng

PD_LEVQUANTS = (0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95)          # dbarts pdbart's default levquants

INT_MAX = 2147483647
EXTRACT_TYPES = ("ev", "ppd", "fixef", "indiv.fixef", "ranef", "indiv.ranef", "indiv.bart", "sigma", "Sigma", "k", "varcount",
                 "stan", "trees", "callback")


def combine_chains_f(x: np.ndarray) -> np.ndarray:
    """reference R/generics.R:1-16: the last two dims (iterations, chains) become one, chain 1's draws first."""
    x = np.asarray(x)
    if x.ndim > 2:
        return np.swapaxes(x, -1, -2).reshape(x.shape[:-2] + (x.shape[-2] * x.shape[-1],))
    if x.ndim == 2:
        return x.T.reshape(-1)
    return x


def _pnorm(x):
    return 0.5 * (1.0 + np.vectorize(math.erf)(np.asarray(x) / math.sqrt(2.0)))


def _theta_to_sigma(theta: np.ndarray, p: int) -> np.ndarray:
    """lme4 mkVarCorr(sc = 1, ...) for one term (reference R/generics.R:248): theta holds the lower triangle of the
    covariance factor column by column, Sigma = L L'."""
    L = np.zeros((p, p))
    k = 0
    for c in range(p):
        for r in range(c, p):
            L[r, c] = theta[k]
            k += 1
    return L @ L.T


@dataclass
class Stan4bartFit:
    family: str
    par_names: list
    stan: np.ndarray            # [num_pars, iterations, chains]
    bart_train: np.ndarray      # [n, iterations, chains]
    bart_test: Optional[np.ndarray]
    bart_varcount: np.ndarray   # [P, iterations, chains]
    warmup: Optional[dict]      # same four arrays for the warmup phase
    X: np.ndarray               # fixed-effect design as given (not centred), [n, K]
    X_means: np.ndarray
    X_test: Optional[np.ndarray]
    terms: list                 # grouping terms in Z column order
    terms_test: Optional[list]
    offset: Optional[np.ndarray]
    offset_test: Optional[np.ndarray]
    offset_type: str
    range_bart: np.ndarray      # [2, chains] (min, max) of the BART response scale
    samplers: list = field(default_factory=list)   # live samplers holding the kept trees (bart_args keepTrees)
    trees: Optional[list] = None
    callback: Optional[np.ndarray] = None   # [len(result), iterations, chains]
    weights: Optional[np.ndarray] = None    # observation weights of the training sample
    k: Optional[np.ndarray] = None          # [iterations, chains] draws of a modeled end-node sensitivity k (bart_args k = chi(...)), else None
    batch_stats: Optional[dict] = None      # batch_chains=True: the sweep groups' counters summed over the thread batches, else None
    latents: str = "exact"                  # how the probit latents were drawn (bart_args latents): "exact" or "parallel"

    # ------------------------------------------------------------------ helpers
    def _get(self, name: str, include_warmup, only_warmup):
        """reference get_samples (R/generics.R:134-166)."""
        cur = getattr(self, name)
        if not include_warmup:
            return cur
        if self.warmup is None or self.warmup.get(name) is None:
            raise ValueError("model was fit without warmup draws kept")
        w = self.warmup[name]
        return w if only_warmup else np.concatenate([w, cur], axis=-2)

    def _rows(self, prefix: str):
        return [i for i, nm in enumerate(self.par_names) if nm.startswith(prefix)]

    @property
    def n_chains(self) -> int:
        return self.bart_train.shape[2]

    def _ranef_arrays(self, include_warmup, only_warmup):
        stan = self._get("stan", include_warmup, only_warmup)
        rows = self._rows("b.")
        b = stan[rows]
        out, base = {}, 0
        for g in self.terms:
            blk = b[base: base + g.p * g.l]                    # level-major, the p coefficients adjacent
            out[g.name] = blk.reshape(g.l, g.p, *blk.shape[1:]).transpose(1, 0, 2, 3)   # [predictor, group, iter, chain]
            base += g.p * g.l
        return out

    def _sigma_arrays(self, include_warmup, only_warmup):
        stan = self._get("stan", include_warmup, only_warmup)
        th = stan[self._rows("theta_L.")]
        out, base = {}, 0
        for g in self.terms:
            k = g.p * (g.p + 1) // 2
            blk = th[base: base + k]
            S = np.zeros((g.p, g.p) + blk.shape[1:])
            for i in range(blk.shape[1]):
                for c in range(blk.shape[2]):
                    S[:, :, i, c] = _theta_to_sigma(blk[:, i, c], g.p)
            out[g.name] = S
            base += k
        return out

    def _fitted_fixed(self, x, include_warmup, only_warmup):
        """reference fitted_fixed (R/generics.R:510-551): x beta - sum(beta * X_means)."""
        fixef = self._get("stan", include_warmup, only_warmup)[self._rows("beta.")]      # [K, iter, chain]
        xc = np.asarray(x, dtype=np.float64).reshape(-1, fixef.shape[0]) - self.X_means
        return np.einsum("nk,ksc->nsc", xc, fixef)

    def _fitted_random(self, terms_new, include_warmup, only_warmup, sample_new_levels, rng):
        """reference fitted_random (R/generics.R:553-606) + levelfun (R/lme4_functions.R:1337-1378)."""
        re = self._ranef_arrays(include_warmup, only_warmup)
        names = {g.name: g for g in self.terms}
        n = len(terms_new[0].levels)
        any_arr = next(iter(re.values()))
        out = np.zeros((n,) + any_arr.shape[2:])
        Sig = None
        for g in terms_new:
            if g.name not in names:
                raise ValueError("grouping factors specified that were not present in original model")
            old = names[g.name]
            if g.p != old.p:
                raise ValueError("random effects specified that were not present in original model")
            b = re[g.name]                                       # [p, l, iter, chain]
            lev = np.asarray(g.levels, dtype=np.int64)
            n_new = int(max(0, lev.max() - old.l))
            if n_new:
                ext = np.zeros((b.shape[0], n_new) + b.shape[2:])
                if sample_new_levels:
                    Sig = Sig or self._sigma_arrays(include_warmup, only_warmup)
                    S = Sig[g.name]
                    for i in range(b.shape[2]):
                        for c in range(b.shape[3]):
                            L = np.linalg.cholesky(S[:, :, i, c] + 1e-300 * np.eye(b.shape[0]))
                            ext[:, :, i, c] = L @ rng.standard_normal((b.shape[0], n_new))
                b = np.concatenate([b, ext], axis=1)
            vals = np.ones((n, g.p))
            if g.p > 1:
                vals[:, 1:] = np.asarray(g.slopes, dtype=np.float64).reshape(n, g.p - 1)
            out += np.einsum("np,pnsc->nsc", vals, b[:, lev - 1])
        return out

    # ------------------------------------------------------------------ extract
    def extract(self, type: str = "ev", sample: str = "train", combine_chains: bool = True, sample_new_levels: bool = True,
                include_warmup=False, seed: Optional[int] = None, **kw):
        if type not in EXTRACT_TYPES:
            raise ValueError(f"'type' must be one of {EXTRACT_TYPES}")
        if type == "trees":
            # reference R/generics.R:186-193: the kept draws' trees (bart_args keepTrees), optionally one draw / some trees;
            # columns chain, sample, tree, n, var (-1 = leaf), value (cut point | leaf mean on the BART scale)
            if not self.samplers:
                raise ValueError("extracting trees requires stan4bart to be called with `bart_args = {'keepTrees': True}`")
            sample_nums, tree_nums, chain_nums = kw.get("sampleNums"), kw.get("treeNums"), kw.get("chainNums")
            cols = {k: [] for k in ("chain", "sample", "tree", "n", "var", "split", "value")}
            for c, smp in enumerate(self.samplers):
                if chain_nums is not None and c not in np.atleast_1d(chain_nums):
                    continue
                # the index vectors go to the C boundary as they are (stan4bart_getTrees takes them: reference src/init.cpp:514-671)
                tr = smp.get_kept_trees_indexed(None if sample_nums is None else np.atleast_1d(sample_nums),
                                                None if tree_nums is None else np.atleast_1d(tree_nums))
                cols["chain"].append(np.full(len(tr["tree"]), c, dtype=np.int32))
                for k in ("sample", "tree", "n", "var", "split", "value"):
                    cols[k].append(tr[k])
            return {k: np.concatenate(v) if v else np.zeros(0) for k, v in cols.items()}
        if sample not in ("train", "test"):
            raise ValueError("'sample' must be 'train' or 'test'")
        if isinstance(include_warmup, str):
            if include_warmup != "only":
                raise ValueError("'include_warmup' must be logical or \"only\"")
            include_warmup, only_warmup = True, True
        else:
            include_warmup, only_warmup = bool(include_warmup), False
        done = (lambda r: ({k: combine_chains_f(v) for k, v in r.items()} if isinstance(r, dict) else combine_chains_f(r))
                if combine_chains else r)
        if type == "callback":
            if self.callback is None:
                raise ValueError("cannot extract callback samples for model fit without callback function")
            return done(self._get("callback", include_warmup, only_warmup))
        is_bernoulli = self.family == "binomial"
        if type == "sigma" and is_bernoulli:
            raise ValueError("cannot extract 'sigma': binary outcome model does not have a residual standard error parameter")
        n_fixef, n_terms = len(self._rows("beta.")), len(self.terms)
        if type == "fixef":
            if not n_fixef:
                raise ValueError("cannot extract fixef for model with no unmodeled parameters")
            return done(self._get("stan", include_warmup, only_warmup)[self._rows("beta.")])
        if type == "ranef":
            if not n_terms:
                raise ValueError("cannot extract ranef for model with no modeled parameters")
            return done(self._ranef_arrays(include_warmup, only_warmup))
        if type == "Sigma":
            if not n_terms:
                raise ValueError("cannot extract Sigma for model with no modeled parameters")
            return done(self._sigma_arrays(include_warmup, only_warmup))
        if type == "sigma":
            return done(self._get("stan", include_warmup, only_warmup)[self.par_names.index("aux.1")])
        if type == "k":      # reference R/generics.R:223-224, 280-284
            if self.k is None:
                raise ValueError("cannot extract 'k': model was not fit with end-node sensitivity as a modeled parameter")
            return done(self._get("k", include_warmup, only_warmup))
        if type == "varcount":
            return done(self._get("bart_varcount", include_warmup, only_warmup))
        if type == "stan":
            return done(self._get("stan", include_warmup, only_warmup))

        rng = np.random.default_rng(seed)
        if sample == "train":
            X, terms, offset = self.X, self.terms, self.offset
        else:
            if self.bart_test is None:
                raise ValueError("model was fit without test data")
            X, terms, offset = self.X_test, self.terms_test, self.offset_test
        ot = self.offset_type
        fix = ran = bart = 0.0
        if type in ("ev", "ppd", "indiv.fixef") and n_fixef:
            if offset is not None and ot in ("fixef", "parametric") and type != "indiv.fixef":
                fix = np.asarray(offset)[:, None, None]
            else:
                fix = self._fitted_fixed(X, include_warmup, only_warmup)
        if type in ("ev", "ppd", "indiv.ranef") and n_terms:
            if offset is not None and ot in ("ranef", "parametric") and type != "indiv.ranef":
                ran = 0.0 if ot == "parametric" else np.asarray(offset)[:, None, None]
            else:
                ran = self._fitted_random(terms, include_warmup, only_warmup, sample_new_levels, rng)
        if type in ("ev", "ppd", "indiv.bart"):
            if offset is not None and ot == "bart" and type != "indiv.bart":
                bart = np.asarray(offset)[:, None, None]
            else:
                bart = self._get("bart_train" if sample == "train" else "bart_test", include_warmup, only_warmup)
        result = {"ev": lambda: bart + fix + ran, "ppd": lambda: bart + fix + ran, "indiv.fixef": lambda: fix,
                  "indiv.ranef": lambda: ran, "indiv.bart": lambda: bart}[type]()
        if np.isscalar(result):
            raise ValueError(f"model has no component for type '{type}'")
        if type in ("ev", "ppd") and offset is not None and ot == "default":
            result = result + np.asarray(offset)[:, None, None]
        if type in ("ev", "ppd") and is_bernoulli:
            result = _pnorm(result)
        if type == "ppd":
            if is_bernoulli:
                result = (rng.random(result.shape) < result).astype(np.float64)
            else:
                sig = self._get("stan", include_warmup, only_warmup)[self.par_names.index("aux.1")]   # [iter, chain]
                sd = sig[None]
                if sample == "train" and self.weights is not None:     # reference R/generics.R:452-459: sd = sigma sqrt(1 / w)
                    sd = sd * np.sqrt(1.0 / self.weights)[:, None, None]
                result = result + rng.standard_normal(result.shape) * sd
        return done(result)

    # ------------------------------------------------------------------ fitted
    def fitted(self, type: str = "ev", sample: str = "train", sample_new_levels: bool = True, seed: Optional[int] = None):
        """reference fitted.stan4bartFit (R/generics.R:486-508): posterior mean over draws and chains."""
        s = self.extract(type, sample, combine_chains=True, sample_new_levels=sample_new_levels, seed=seed)
        avg = lambda x: np.mean(x, axis=-1)
        return {k: avg(v) for k, v in s.items()} if isinstance(s, dict) else avg(s)

    # ------------------------------------------------------------------ predict
    def predict(self, x_bart=None, X=None, groups: Optional[Sequence[GroupTerm]] = None, offset=None, type: str = "ev",
                combine_chains: bool = True, sample_new_levels: bool = True, seed: Optional[int] = None):
        """reference predict.stan4bartFit (R/generics.R:608-724); BART part from the kept trees
        (``stan4bart_predictBART``, reference src/init.cpp:354-403) — needs bart_args keepTrees."""
        if type not in ("ev", "ppd", "indiv.fixef", "indiv.ranef", "indiv.bart"):
            raise ValueError("'type' must be one of ev, ppd, indiv.fixef, indiv.ranef, indiv.bart")
        if x_bart is None and X is None and groups is None:
            return self.extract(type, combine_chains=combine_chains)
        rng = np.random.default_rng(seed)
        is_bernoulli = self.family == "binomial"
        n_fixef, n_terms = len(self._rows("beta.")), len(self.terms)
        fix = ran = bart = 0.0
        if type in ("ev", "ppd", "indiv.fixef"):
            if X is not None and n_fixef:
                fix = self._fitted_fixed(X, False, False)
            elif type == "indiv.fixef":
                raise ValueError("predict called with type 'indiv.fixef', but model does not include fixed effect terms")
        if type in ("ev", "ppd", "indiv.bart"):
            if not self.samplers:
                raise ValueError("predict for bart components requires 'bart_args' to contain 'keepTrees' as True")
            bart = np.stack([s.predict_bart(np.asarray(x_bart, dtype=np.float64)) for s in self.samplers], axis=2)
        if type in ("ev", "ppd", "indiv.ranef"):
            if groups is not None and len(groups) and n_terms:
                order = {g.name: g for g in groups}
                ran = self._fitted_random([order[g.name] for g in self.terms if g.name in order], False, False, sample_new_levels, rng)
            elif type == "indiv.ranef":
                raise ValueError("predict called with type 'indiv.ranef', but model does not include random effect terms")
        off = 0.0 if offset is None else np.asarray(offset, dtype=np.float64)[:, None, None]
        result = {"ev": lambda: bart + fix + ran + off, "ppd": lambda: bart + fix + ran + off, "indiv.fixef": lambda: fix,
                  "indiv.ranef": lambda: ran, "indiv.bart": lambda: bart}[type]()
        if type in ("ev", "ppd") and is_bernoulli:
            result = _pnorm(result)
        if type == "ppd":
            if is_bernoulli:
                result = (rng.random(result.shape) < result).astype(np.float64)
            else:
                sig = self.stan[self.par_names.index("aux.1")]
                result = result + rng.standard_normal(result.shape) * sig[None]
        return combine_chains_f(result) if combine_chains else result

    # ------------------------------------------------------------------ predict_summary
    def _ell_random(self, terms_new, sample_new_levels, rng):
        """The random part of ``_fitted_random`` as an ELL table over the rows: (ell_index [n x E] int32, ell_value [n x E], coefficient tables
        [chain][draws x q']).  One entry per term and slope (E = sum of the terms' p): its column is the coefficient's position in the chain's ``b``
        table (level-major, the p coefficients of a level adjacent); unseen levels are appended as extra columns and drawn per draw exactly as
        ``_fitted_random`` draws them (the same generator calls in the same order); with ``sample_new_levels=False`` their entries are padding
        (index -1: they contribute nothing)."""
        stan = self._get("stan", False, False)
        b_all = stan[self._rows("b.")]                               # [q, iter, chain]
        q, n_iter, n_chain = b_all.shape
        names = {g.name: g for g in self.terms}
        base, at = {}, 0
        for g in self.terms:
            base[g.name] = at
            at += g.p * g.l
        n = len(terms_new[0].levels)
        idx_cols, val_cols, extra = [], [], []                       # extra: [p * n_new, iter, chain] blocks appended after the q columns
        n_extra, Sig = 0, None
        for g in terms_new:
            if g.name not in names:
                raise ValueError("grouping factors specified that were not present in original model")
            old = names[g.name]
            if g.p != old.p:
                raise ValueError("random effects specified that were not present in original model")
            lev = np.asarray(g.levels, dtype=np.int64)
            n_new = int(max(0, lev.max() - old.l))
            seen = lev <= old.l
            col0 = np.where(seen, base[g.name] + (lev - 1) * g.p, -1)
            if n_new:
                if sample_new_levels:
                    Sig = Sig or self._sigma_arrays(False, False)
                    S = Sig[g.name]
                    ext = np.zeros((g.p, n_new, n_iter, n_chain))
                    for i in range(n_iter):
                        for c in range(n_chain):
                            L = np.linalg.cholesky(S[:, :, i, c] + 1e-300 * np.eye(g.p))
                            ext[:, :, i, c] = L @ rng.standard_normal((g.p, n_new))
                    extra.append(ext.transpose(1, 0, 2, 3).reshape(n_new * g.p, n_iter, n_chain))      # level-major, like b
                    col0 = np.where(seen, col0, q + n_extra + (lev - old.l - 1) * g.p)
                    n_extra += n_new * g.p
            vals = np.ones((n, g.p))
            if g.p > 1:
                vals[:, 1:] = np.asarray(g.slopes, dtype=np.float64).reshape(n, g.p - 1)
            for j in range(g.p):
                idx_cols.append(np.where(col0 >= 0, col0 + j, -1))
                val_cols.append(vals[:, j])
        table = np.concatenate([b_all] + extra, axis=0) if extra else b_all
        coef = [np.ascontiguousarray(table[:, :, c].T) for c in range(n_chain)]
        return np.column_stack(idx_cols).astype(np.int32), np.column_stack(val_cols), coef

    @staticmethod
    def _pool_chains(parts):
        """(count, mean, m2) of several chains pooled pairwise (Chan et al.): O(rows x chains)."""
        n, mean, m2 = parts[0]
        mean, m2 = mean.copy(), m2.copy()
        for nb, mb, m2b in parts[1:]:
            d = mb - mean
            tot = n + nb
            mean = mean + d * (nb / tot)
            m2 = m2 + m2b + d * d * (n * nb / tot)
            n = tot
        return n, mean, m2

    def _summary_linear(self, type, X, groups, offset, sample_new_levels, rng):
        """The linear parts and the link of a ``predict_summary`` / ``partial_dependence`` call: a function chain -> keyword arguments of the
        sampler's method (fixed part ``dense = X - X_means`` with ``beta``, random part as ``_ell_random``'s table, the offset; "indiv.bart": none)."""
        ev = type == "ev"
        n_fixef, n_terms, n_chain = len(self._rows("beta.")), len(self.terms), len(self.samplers)
        dense = dense_coef = ell_index = ell_value = ell_coef = None
        if ev and X is not None and n_fixef:
            beta = self.stan[self._rows("beta.")]                    # [K, iter, chain]
            dense = np.asarray(X, dtype=np.float64).reshape(-1, n_fixef) - self.X_means
            dense_coef = [np.ascontiguousarray(beta[:, :, c].T) for c in range(n_chain)]
        if ev and groups is not None and len(groups) and n_terms:
            order = {g.name: g for g in groups}
            ell_index, ell_value, ell_coef = self._ell_random([order[g.name] for g in self.terms if g.name in order], sample_new_levels, rng)
        link = 1 if (ev and self.family == "binomial") else 0
        return lambda c: dict(offset=offset if ev else None, dense=dense, dense_coef=None if dense is None else dense_coef[c], ell_index=ell_index,
                              ell_value=ell_value, ell_coef=None if ell_index is None else ell_coef[c], link=link)

    def predict_summary(self, x_bart=None, X=None, groups: Optional[Sequence[GroupTerm]] = None, offset=None, type: str = "ev", row_weights=None,
                        combine_chains: bool = True, sample_new_levels: bool = True, seed: Optional[int] = None):
        """What users take from ``predict``'s [rows x draws] matrix, formed on the device without it (``s4b_predict_summary``, one call per chain):
        ``mean`` and ``sd`` (ddof 1) per row over all draws and chains, and ``average`` [G, iter, chain] — per draw, ``row_weights`` [G x rows]
        (G <= 8, used as given; None: one vector of 1 / rows, the sample average) applied to the rows: sample and subgroup average effects.
        ``type`` "ev" or "indiv.bart"; for a given ``seed`` the draws of unseen levels are ``predict``'s.  Needs bart_args keepTrees."""
        if type == "ppd":
            raise ValueError("predict_summary does not form 'ppd': its noise is drawn per element of the draws matrix (use predict)")
        if type not in ("ev", "indiv.bart"):
            raise ValueError("'type' must be one of ev, indiv.bart (indiv.fixef and indiv.ranef need no trees: use predict)")
        if not self.samplers:
            raise ValueError("predict_summary requires 'bart_args' to contain 'keepTrees' as True")
        if x_bart is None:
            raise ValueError("predict_summary needs x_bart, the new rows of the BART predictors")
        x_bart = np.asarray(x_bart, dtype=np.float64)
        rows = x_bart.shape[0]
        if row_weights is None:
            w = np.full((1, rows), 1.0 / rows)
        else:
            w = np.asarray(row_weights, dtype=np.float64)
            if w.ndim != 2 or w.shape[1] != rows:
                raise ValueError(f"row_weights must have shape [G, {rows}], not {w.shape}")
            if not 1 <= w.shape[0] <= 8:
                raise ValueError(f"row_weights holds {w.shape[0]} weight vectors: between 1 and 8 per call")
        linear = self._summary_linear(type, X, groups, offset, sample_new_levels, np.random.default_rng(seed))
        parts, avgs = [], []
        for c, smp in enumerate(self.samplers):
            r = smp.predict_summary(x_bart, weights=w, **linear(c))
            parts.append((r["draws"], r["mean"], r["m2"]))
            avgs.append(r["average"].T)                              # [G, iter]
        n, mean, m2 = self._pool_chains(parts)
        sd = np.sqrt(m2 / (n - 1)) if n > 1 else np.full(rows, np.nan)
        average = np.stack(avgs, axis=2)
        return {"mean": mean, "sd": sd, "draws": int(n), "average": combine_chains_f(average) if combine_chains else average}

    # ------------------------------------------------------------------ partial_dependence
    @staticmethod
    def pd_default_grid(column):
        """dbarts' ``levquants`` of a column: its 0.05, 0.1, 0.2 ... 0.9, 0.95 quantiles (numpy's default interpolation, R's type 7)."""
        return np.quantile(np.asarray(column, dtype=np.float64), PD_LEVQUANTS)

    def partial_dependence(self, var, x_bart=None, grid=None, X=None, groups: Optional[Sequence[GroupTerm]] = None, offset=None, type: str = "ev",
                           row_weights=None, probs=(0.025, 0.975), combine_chains: bool = True, sample_new_levels: bool = True,
                           seed: Optional[int] = None):
        """The partial dependence function of one BART predictor (``var`` an index into ``x_bart``'s columns) or of two jointly (a pair of indices):
        per draw, the (weighted) average over the rows of the prediction with the predictor(s) set to each grid value — dbarts' ``pdbart`` /
        ``pd2bart`` — in one fused device call per chain and 64 grid points (``s4b_partial_dependence``) instead of one ``predict`` per grid value.
        ``grid`` None: the ``levquants`` quantiles of the column(s) of ``x_bart`` (a pair: their product, first predictor slowest); one predictor:
        [G] values; a pair: [G x 2] points, or a tuple of two vectors whose product is taken.  The fixed and random parts are ``predict_summary``'s and
        stay at the rows' own values.  ``row_weights`` None (the sample average) or [rows].  Returns ``grid``, ``pd`` [G, draws] ([G, iter, chain]
        with ``combine_chains=False``) and ``mean``, ``lower``, ``upper`` [G]: mean and the ``probs`` quantiles over all draws and chains."""
        if type == "ppd":
            raise ValueError("partial_dependence does not form 'ppd': its noise is drawn per element of the draws matrix (use predict)")
        if type not in ("ev", "indiv.bart"):
            raise ValueError("'type' must be one of ev, indiv.bart (indiv.fixef and indiv.ranef need no trees: use predict)")
        if not self.samplers:
            raise ValueError("partial_dependence requires 'bart_args' to contain 'keepTrees' as True")
        if x_bart is None:
            raise ValueError("partial_dependence needs x_bart, the rows of the BART predictors to average over")
        x_bart = np.asarray(x_bart, dtype=np.float64)
        rows, P = x_bart.shape
        vs = [int(v) for v in np.atleast_1d(var)]
        if len(vs) not in (1, 2) or len(set(vs)) != len(vs) or not all(0 <= v < P for v in vs):
            raise ValueError(f"'var' must be one column index of x_bart or two different ones in [0, {P}), not {var!r}")
        if grid is None:
            grid = tuple(self.pd_default_grid(x_bart[:, v]) for v in vs)
            grid = grid[0] if len(vs) == 1 else grid
        if isinstance(grid, tuple):
            if len(grid) != 2 or len(vs) != 2:
                raise ValueError("a tuple of grid vectors is the product grid of a pair of predictors")
            a, b = (np.asarray(t, dtype=np.float64).ravel() for t in grid)
            grid = np.column_stack([np.repeat(a, len(b)), np.tile(b, len(a))])
        grid = np.asarray(grid, dtype=np.float64)
        pts = grid.reshape(-1, 1) if grid.ndim == 1 else grid
        if pts.ndim != 2 or pts.shape[1] != len(vs) or not len(pts):
            raise ValueError(f"grid must hold at least one point of {len(vs)} value(s), not shape {grid.shape}")
        if np.isnan(pts).any():
            raise ValueError("grid holds a NaN")
        w = None
        if row_weights is not None:
            w = np.asarray(row_weights, dtype=np.float64)
            if w.shape != (rows,):
                raise ValueError(f"row_weights must have shape [{rows}], not {w.shape}")
        linear = self._summary_linear(type, X, groups, offset, sample_new_levels, np.random.default_rng(seed))
        per_chain = []
        for c, smp in enumerate(self.samplers):
            args = linear(c)
            pieces = [smp.partial_dependence(x_bart, vs, pts[g0:g0 + PD_GRID_MAX], weights=w, **args)["pd"] for g0 in range(0, len(pts), PD_GRID_MAX)]
            per_chain.append(np.concatenate(pieces, axis=1).T)                   # [G, iter]
        pd = np.stack(per_chain, axis=2)
        flat = combine_chains_f(pd)
        lower, upper = np.quantile(flat, probs, axis=1)
        return {"grid": grid, "pd": flat if combine_chains else pd, "mean": flat.mean(axis=1), "lower": lower, "upper": upper}

    # ------------------------------------------------------------------ predict_curves
    def predict_curves(self, var, x_bart=None, grid=None, X=None, groups: Optional[Sequence[GroupTerm]] = None, offset=None, anchor=None,
                       probs=(0.025, 0.5, 0.975), type: str = "ev", sample_new_levels: bool = True, seed: Optional[int] = None):
        """The individual conditional expectation curves of one BART predictor (``var`` an index into ``x_bart``'s columns) or of two jointly:
        per row and grid value the prediction with the predictor(s) set to that value — ``partial_dependence`` before its average over the rows —
        summarised on the device in ONE pooled call over all chains (``s4b_predict_curves``) without any [rows x draws] matrix.  ``grid`` as
        ``partial_dependence`` takes it, at most 64 points (None: ``pd_default_grid`` of the column(s) of ``x_bart``).  ``anchor`` None or a grid
        index: the curves are centred there, c = v - v(anchor) per draw — the effect of each grid value against the anchor's for this row, with
        its own interval.  The fixed and random parts are ``predict_summary``'s and stay at the rows' own values.  Returns ``grid``; ``mean``,
        ``sd`` (ddof 1), ``p_max``, ``p_min`` [rows, G] — the share of the draws in which a grid point is the row's highest / lowest (the lowest
        index on an exact tie); ``quantiles`` [Q, rows, G]; ``range`` = dict(mean, sd, quantiles [Q, rows]) of max - min over the grid within
        a draw; ``draws``, the pooled count, and ``info``."""
        if type == "ppd":
            raise ValueError("predict_curves does not form 'ppd': its noise is drawn per element of the draws matrix (use predict)")
        if type not in ("ev", "indiv.bart"):
            raise ValueError("'type' must be one of ev, indiv.bart (indiv.fixef and indiv.ranef need no trees: use predict)")
        if not self.samplers:
            raise ValueError("predict_curves requires 'bart_args' to contain 'keepTrees' as True")
        if x_bart is None:
            raise ValueError("predict_curves needs x_bart, the rows of the BART predictors")
        x_bart = np.asarray(x_bart, dtype=np.float64)
        rows, P = x_bart.shape
        vs = [int(v) for v in np.atleast_1d(var)]
        if len(vs) not in (1, 2) or len(set(vs)) != len(vs) or not all(0 <= v < P for v in vs):
            raise ValueError(f"'var' must be one column index of x_bart or two different ones in [0, {P}), not {var!r}")
        if grid is None:
            grid = tuple(self.pd_default_grid(x_bart[:, v]) for v in vs)
            grid = grid[0] if len(vs) == 1 else grid
        if isinstance(grid, tuple):
            if len(grid) != 2 or len(vs) != 2:
                raise ValueError("a tuple of grid vectors is the product grid of a pair of predictors")
            a, b = (np.asarray(t, dtype=np.float64).ravel() for t in grid)
            grid = np.column_stack([np.repeat(a, len(b)), np.tile(b, len(a))])
        grid = np.asarray(grid, dtype=np.float64)
        pts = grid.reshape(-1, 1) if grid.ndim == 1 else grid
        if pts.ndim != 2 or pts.shape[1] != len(vs) or not len(pts):
            raise ValueError(f"grid must hold at least one point of {len(vs)} value(s), not shape {grid.shape}")
        if len(pts) > PD_GRID_MAX:
            raise ValueError(f"grid holds {len(pts)} points, at most {PD_GRID_MAX} per call (the extremes need the whole grid at once)")
        if np.isnan(pts).any():
            raise ValueError("grid holds a NaN")
        if anchor is not None and not 0 <= int(anchor) < len(pts):
            raise ValueError(f"'anchor' must be None or a grid index in [0, {len(pts)}), not {anchor!r}")
        pr = np.atleast_1d(np.asarray(probs, dtype=np.float64))
        if pr.ndim != 1 or not np.all((pr >= 0.0) & (pr <= 1.0)):
            raise ValueError(f"'probs' must be a vector of values in [0, 1], not {probs!r}")
        outputs = tuple(k for k in CURVES_OUTPUTS if len(pr) or "quantiles" not in k)
        linear = self._summary_linear(type, X, groups, offset, sample_new_levels, np.random.default_rng(seed))
        first, others = linear(0), [linear(c) for c in range(1, len(self.samplers))]
        r = self.samplers[0].predict_curves(x_bart, vs, pts, anchor=anchor, probs=pr, outputs=outputs, peers=self.samplers[1:],
                                            peer_dense_coef=None if first["dense"] is None else [a["dense_coef"] for a in others],
                                            peer_ell_coef=None if first["ell_index"] is None else [a["ell_coef"] for a in others], **first)
        n = r["draws"]
        sd = lambda m2: np.sqrt(m2 / (n - 1)) if n > 1 else np.full(m2.shape, np.nan)
        return {"grid": grid, "mean": r["mean"], "sd": sd(r["m2"]), "p_max": r["p_max"], "p_min": r["p_min"], "quantiles": r["quantiles"], "probs": pr,
                "range": {"mean": r["range_mean"], "sd": sd(r["range_m2"]), "quantiles": r["range_quantiles"]}, "draws": n, "info": r["info"]}

    # ------------------------------------------------------------------ predict_quantiles
    def predict_quantiles(self, x_bart=None, X=None, groups: Optional[Sequence[GroupTerm]] = None, offset=None, type: str = "ev",
                          probs=(0.025, 0.5, 0.975), sample_new_levels: bool = True, seed: Optional[int] = None):
        """The per-row credible interval — ``apply(extract(fit), 1, quantile, probs)`` — formed on the device without ``predict``'s [rows x draws]
        matrix: the ``probs`` quantiles (R's type 7) of the expected value of each row over all draws and chains, in ONE pooled call
        (``s4b_predict_quantiles``: the first chain's sampler with the others as its peers; quantiles of chains cannot be merged afterwards).
        ``type`` "ev" or "indiv.bart"; for a given ``seed`` the draws of unseen levels are ``predict``'s.  Needs bart_args keepTrees.
        Returns ``probs``, ``quantiles`` [Q, rows] and ``draws``, the pooled count."""
        if type == "ppd":
            raise ValueError("predict_quantiles does not form 'ppd': its noise is drawn per element of the draws matrix (use predict)")
        if type not in ("ev", "indiv.bart"):
            raise ValueError("'type' must be one of ev, indiv.bart (indiv.fixef and indiv.ranef need no trees: use predict)")
        if not self.samplers:
            raise ValueError("predict_quantiles requires 'bart_args' to contain 'keepTrees' as True")
        if x_bart is None:
            raise ValueError("predict_quantiles needs x_bart, the new rows of the BART predictors")
        pr = np.atleast_1d(np.asarray(probs, dtype=np.float64))
        if pr.ndim != 1 or not len(pr) or not np.all((pr >= 0.0) & (pr <= 1.0)):
            raise ValueError(f"'probs' must be a vector of values in [0, 1], not {probs!r}")
        x_bart = np.asarray(x_bart, dtype=np.float64)
        linear = self._summary_linear(type, X, groups, offset, sample_new_levels, np.random.default_rng(seed))
        first, others = linear(0), [linear(c) for c in range(1, len(self.samplers))]
        r = self.samplers[0].predict_quantiles(x_bart, pr, peers=self.samplers[1:],
                                               peer_dense_coef=None if first["dense"] is None else [a["dense_coef"] for a in others],
                                               peer_ell_coef=None if first["ell_index"] is None else [a["ell_coef"] for a in others], **first)
        return {"probs": pr, "quantiles": r["quantiles"], "draws": r["draws"]}

    # ------------------------------------------------------------------ predict_contrast
    def predict_contrast(self, x_bart=None, x_bart0=None, X=None, X0=None, groups: Optional[Sequence[GroupTerm]] = None,
                         groups0: Optional[Sequence[GroupTerm]] = None, offset=None, offset0=None, treatment=None, levels=(1.0, 0.0), type: str = "ev",
                         row_weights=None, probs=(0.025, 0.5, 0.975), combine_chains: bool = True, sample_new_levels: bool = True,
                         seed: Optional[int] = None):
        """Per-row treatment effects — ``(predict(arm 1) - predict(arm 0))`` of the same rows under the same draws, the reference's
        ``samples.icate`` — summarised on the device without either [rows x draws] matrix, in ONE pooled call (``s4b_predict_contrast``: the first
        chain's sampler with the others as its peers).  Arm 1 is ``x_bart``, ``X``, ``groups``, ``offset``; arm 0 the arguments with suffix 0,
        each None for arm 1's.  ``treatment=("x_bart" | "X", column)`` builds both arms from the one row set given, the column set to
        ``levels[0]`` in arm 1 and ``levels[1]`` in arm 0 (slopes of ``groups`` are not touched: hand random slopes on the treatment in as explicit
        arms).  The arms may differ in at most two BART columns.  The random parts of both arms share one coefficient table and one draw of every
        unseen level.  ``type`` "ev" or "indiv.bart".  ``row_weights`` [G x rows], G <= 8 (None: 1 / rows, the sample average effect).
        Returns ``mean`` and ``sd`` (ddof 1) per row, ``average`` [G, draws] ([G, iter, chain] with ``combine_chains=False``), ``probs``,
        ``quantiles`` [Q, rows] and ``draws``."""
        if type == "ppd":
            raise ValueError("predict_contrast does not form 'ppd': its noise is drawn per element of the draws matrix (use predict)")
        if type not in ("ev", "indiv.bart"):
            raise ValueError("'type' must be one of ev, indiv.bart (indiv.fixef and indiv.ranef need no trees: use predict)")
        if not self.samplers:
            raise ValueError("predict_contrast requires 'bart_args' to contain 'keepTrees' as True")
        if x_bart is None:
            raise ValueError("predict_contrast needs x_bart, the new rows of the BART predictors")
        pr = np.atleast_1d(np.asarray(probs, dtype=np.float64))
        if pr.ndim != 1 or len(pr) > 16 or not np.all((pr >= 0.0) & (pr <= 1.0)):
            raise ValueError(f"'probs' must be a vector of at most 16 values in [0, 1], not {probs!r}")
        x_bart, x_bart0, kw, peer_kw = self._contrast_arms(x_bart, x_bart0, X, X0, groups, groups0, offset, offset0, treatment, levels, type,
                                                           sample_new_levels, seed)
        rows = x_bart.shape[0]
        if row_weights is None:
            w = np.full((1, rows), 1.0 / rows)
        else:
            w = np.asarray(row_weights, dtype=np.float64)
            if w.ndim != 2 or w.shape[1] != rows:
                raise ValueError(f"row_weights must have shape [G, {rows}], not {w.shape}")
            if not 1 <= w.shape[0] <= 8:
                raise ValueError(f"row_weights holds {w.shape[0]} weight vectors: between 1 and 8 per call")
        r = self.samplers[0].predict_contrast(x_bart, x_bart0, probs=pr, weights=w, **peer_kw, **kw)
        n = r["draws"]
        sd = np.sqrt(r["m2"] / (n - 1)) if n > 1 else np.full(rows, np.nan)
        average = r["average"].T                                     # [G, pooled draws], chain after chain
        if not combine_chains:
            average = average.reshape(w.shape[0], len(self.samplers), -1).transpose(0, 2, 1)
        return {"mean": r["mean"], "sd": sd, "average": average, "probs": pr, "quantiles": r["quantiles"], "draws": n}

    def _contrast_arms(self, x_bart, x_bart0, X, X0, groups, groups0, offset, offset0, treatment, levels, type, sample_new_levels, seed):
        """The arms of a ``predict_contrast`` or ``predict_groups`` call as the pooled sampler call takes them: (x_bart, x_bart0, the keyword arguments
        of the first chain's sampler — the link, the row side of both arms, its coefficient tables — and those naming the other chains as its peers).
        Without any arm-0 argument and without ``treatment`` nothing of arm 0 is in them: one arm, formed as ``predict_quantiles`` forms it."""
        x_bart = np.asarray(x_bart, dtype=np.float64)
        rows = x_bart.shape[0]
        if treatment is not None:
            if any(a is not None for a in (x_bart0, X0, groups0, offset0)):
                raise ValueError("'treatment' builds both arms from one row set: no explicit arm-0 argument (x_bart0, X0, groups0, offset0) beside it")
            if not (isinstance(treatment, (tuple, list)) and len(treatment) == 2 and treatment[0] in ("x_bart", "X")) or len(levels) != 2:
                raise ValueError(f"'treatment' must be (\"x_bart\" | \"X\", column) and 'levels' a pair, not {treatment!r}, {levels!r}")
            where, col = treatment[0], int(treatment[1])
            src = x_bart if where == "x_bart" else (None if X is None else np.asarray(X, dtype=np.float64).reshape(rows, -1))
            if src is None or not 0 <= col < src.shape[1]:
                raise ValueError(f"'treatment' names column {col} of {where}, which is not there")
            arm1, arm0 = src.copy(), src.copy()
            arm1[:, col], arm0[:, col] = float(levels[0]), float(levels[1])
            if where == "x_bart":
                x_bart, x_bart0 = arm1, arm0
            else:
                X, X0 = arm1, arm0
        ev = type == "ev"
        if ev and X0 is not None and X is None:
            raise ValueError("X0 given without X")
        if ev and groups0 is not None and len(groups0) and not (groups is not None and len(groups)):
            raise ValueError("groups0 given without groups")
        if ev and offset0 is not None and offset is None:
            raise ValueError("offset0 given without offset")
        n_fixef, n_terms, n_chain = len(self._rows("beta.")), len(self.terms), len(self.samplers)
        kw = dict(link=1 if (ev and self.family == "binomial") else 0, offset=offset if ev else None, offset0=offset0 if ev else None)
        dense_coef = ell_coef = None
        if ev and X is not None and n_fixef:          # the fixed part: the arms' rows against the one table of the chain
            beta = self.stan[self._rows("beta.")]                    # [K, iter, chain]
            dense_coef = [np.ascontiguousarray(beta[:, :, c].T) for c in range(n_chain)]
            kw.update(dense=np.asarray(X, dtype=np.float64).reshape(-1, n_fixef) - self.X_means, dense_coef=dense_coef[0],
                      dense0=None if X0 is None else np.asarray(X0, dtype=np.float64).reshape(-1, n_fixef) - self.X_means)
        if ev and groups is not None and len(groups) and n_terms:
            # the random parts of both arms through ONE _ell_random call on the stacked rows: one coefficient table, one draw of every unseen level
            terms, two = {g.name: g for g in groups}, groups0 is not None and len(groups0) > 0
            if two:
                by0 = {g.name: g for g in groups0}
                if sorted(by0) != sorted(terms):
                    raise ValueError("groups0 must name the grouping terms of groups")
                terms = {name: GroupTerm(np.concatenate([np.asarray(g.levels), np.asarray(by0[name].levels)]),
                                         None if g.slopes is None else np.vstack([np.asarray(g.slopes, dtype=np.float64).reshape(rows, -1),
                                                                                  np.asarray(by0[name].slopes, dtype=np.float64).reshape(rows, -1)]), name)
                         for name, g in terms.items()}
            ix, val, ell_coef = self._ell_random([terms[g.name] for g in self.terms if g.name in terms], sample_new_levels, np.random.default_rng(seed))
            kw.update(ell_index=ix[:rows], ell_value=val[:rows], ell_coef=ell_coef[0])
            if two:
                kw.update(ell_index0=ix[rows:], ell_value0=val[rows:])
        peer_kw = dict(peers=self.samplers[1:], peer_dense_coef=None if dense_coef is None else dense_coef[1:],
                       peer_ell_coef=None if ell_coef is None else ell_coef[1:])
        return x_bart, None if x_bart0 is None else np.asarray(x_bart0, dtype=np.float64), kw, peer_kw

    # ------------------------------------------------------------------ predict_groups
    ROW_SIDE = ("offset", "offset0", "dense", "dense0", "ell_index", "ell_index0", "ell_value", "ell_value0")          # what is permuted with the rows

    @staticmethod
    def groups_split(n_levels: int, draws: int, limit: int):
        """The consecutive level ranges [(first, end)] of ``predict_groups``' calls: one call where ``limit`` bytes hold the level matrix (8 bytes
        per level and pooled draw), else one level fewer per call than they hold: a range that starts inside a slab of 64 rows takes the rows in
        front of it in that slab along as a level of their own."""
        per = int(limit) // (8 * int(draws))
        if per < 1:
            raise ValueError(f"level_bytes {limit} does not hold one level of {draws} pooled draws ({8 * draws} bytes)")
        if n_levels <= per:
            return [(0, n_levels)]
        if per < 2:
            raise ValueError(f"level_bytes {limit} holds one level of {draws} pooled draws: a split needs room for two (the rows in front of a range keep a level of their own)")
        return [(l0, min(n_levels, l0 + per - 1)) for l0 in range(0, n_levels, per - 1)]

    def predict_groups(self, by, x_bart=None, x_bart0=None, X=None, X0=None, groups: Optional[Sequence[GroupTerm]] = None,
                       groups0: Optional[Sequence[GroupTerm]] = None, offset=None, offset0=None, treatment=None, levels=(1.0, 0.0), type: str = "ev",
                       row_weights=None, statistic: str = "mean", probs=(0.025, 0.5, 0.975), threshold=None, return_draws: bool = False,
                       combine_chains: bool = True, sample_new_levels: bool = True, seed: Optional[int] = None, level_bytes: Optional[int] = None):
        """Per-level averages — the group-by over the rows of ``predict``'s matrix or of ``predict_contrast``'s effects: the average fitted value of
        every school, the average treatment effect of every site with its interval and the posterior probability that it is positive — formed on
        the device without a [rows x draws] matrix (``s4b_predict_groups``: the first chain's sampler with the others as its peers).  ``by`` is a
        label per row (any dtype ``np.unique`` takes, any order) or the NAME of a grouping term in ``groups``, whose level per row is taken.  Any
        arm-0 argument (suffix 0) or ``treatment`` makes it the contrast of two arms, formed as ``predict_contrast`` forms it; otherwise the one
        arm's expected value as ``predict_quantiles`` forms it.  ``row_weights`` None (1) or [rows], non-negative; ``statistic`` "mean" (the
        weighted mean of the level's rows per draw) or "sum".  Where the level matrix (8 bytes per level and pooled draw) exceeds ``level_bytes``
        (None: the library's 1 GiB) the levels are split into consecutive ranges, one call each: the rows are sorted by level, a range is a slice,
        and only the rows between the slab edge in front of a range and its first row (63 at most) are walked a second time: that keeps the slabs
        of the sums where one call has them, so a split returns the bits of one call.  Returns ``levels`` (the unique labels), ``count``, ``weight``, ``mean`` and ``sd`` (ddof 1) over all draws and
        chains, ``probs`` and ``quantiles`` [Q, L], ``p_above`` (with ``threshold``: the share of the draws strictly above it), ``draws`` (the
        pooled count) and, with ``return_draws``, ``average`` [L, draws] ([L, iter, chain] with ``combine_chains=False``).  A level whose weights
        are all 0 has NaN under "mean"."""
        if type == "ppd":
            raise ValueError("predict_groups does not form 'ppd': its noise is drawn per element of the draws matrix (use predict)")
        if type not in ("ev", "indiv.bart"):
            raise ValueError("'type' must be one of ev, indiv.bart (indiv.fixef and indiv.ranef need no trees: use predict)")
        if not self.samplers:
            raise ValueError("predict_groups requires 'bart_args' to contain 'keepTrees' as True")
        if x_bart is None:
            raise ValueError("predict_groups needs x_bart, the new rows of the BART predictors")
        if statistic not in GROUPS_STATISTICS:
            raise ValueError(f"'statistic' must be one of {', '.join(GROUPS_STATISTICS)}, not {statistic!r}")
        pr = np.atleast_1d(np.asarray(probs, dtype=np.float64))
        if pr.ndim != 1 or len(pr) > 16 or not np.all((pr >= 0.0) & (pr <= 1.0)):
            raise ValueError(f"'probs' must be a vector of at most 16 values in [0, 1], not {probs!r}")
        if threshold is not None and np.isnan(float(threshold)):
            raise ValueError("'threshold' is a NaN")
        rows = np.shape(x_bart)[0]
        if isinstance(by, str):
            named = {g.name: g for g in (groups or ())}
            if by not in named:
                raise ValueError(f"'by' names the grouping term {by!r}, which is not in 'groups'")
            by = np.asarray(named[by].levels)
        by = np.asarray(by)
        if by.shape != (rows,):
            raise ValueError(f"'by' must hold one label per row ({rows}), not shape {by.shape}")
        labels, code = np.unique(by, return_inverse=True)
        w = None
        if row_weights is not None:
            w = np.asarray(row_weights, dtype=np.float64)
            if w.shape != (rows,) or not np.all(np.isfinite(w)) or np.any(w < 0.0):
                raise ValueError(f"row_weights must be [{rows}] finite non-negative values")
        two = treatment is not None or any(a is not None for a in (x_bart0, X0, groups0, offset0))
        x_bart, x_bart0, kw, peer_kw = self._contrast_arms(x_bart, x_bart0, X, X0, groups, groups0, offset, offset0, treatment, levels, type,
                                                           sample_new_levels, seed)
        first = self.samplers[0]
        order, code = Sampler.group_order(code.reshape(-1))
        row_side = dict(x_test=x_bart, x_test0=x_bart0, weights=w, **{k: kw.pop(k, None) for k in self.ROW_SIDE})
        row_side = {k: None if a is None else np.asarray(a)[order] for k, a in row_side.items()}
        S = first.groups_draws() + sum(p.groups_draws() for p in peer_kw["peers"])
        L = len(labels)
        out = dict(mean=np.zeros(L), m2=np.zeros(L), weight=np.zeros(L), count=np.zeros(L, dtype=np.int64), quantiles=np.zeros((len(pr), L)),
                   p_above=None if threshold is None else np.zeros(L), draws=np.zeros((L, S)) if return_draws else None)
        start = np.searchsorted(code, np.arange(L + 1))                              # the first sorted row of every level
        for l0, l1 in self.groups_split(L, S, GROUPS_LEVEL_BYTES_MAX if level_bytes is None else level_bytes):
            # the sums are folded over slabs of 64 rows counted from a call's first row: a range starts on the slab edge at or in front of its first
            # row, so that its slabs lie where one call over all rows has them (the same bits); the rows in front, 63 at most, are level 0 and dropped
            i0, i1 = int(start[l0]), int(start[l1])
            p0 = i0 - i0 % 64
            lead = 1 if i0 > p0 else 0
            lab = np.r_[np.zeros(i0 - p0, dtype=code.dtype), code[i0:i1] - l0 + lead]
            r = first.predict_groups(level=lab, n_levels=l1 - l0 + lead, n_arms=2 if two else 1, statistic=statistic, threshold=threshold, probs=pr,
                                     outputs=("mean", "m2", "weight", "count") + (("draws",) if return_draws else ()), presorted=True,
                                     **{k: None if a is None else a[p0:i1] for k, a in row_side.items()}, **peer_kw, **kw)
            for k in ("mean", "m2", "weight", "count", "p_above", "draws"):
                if out[k] is not None:
                    out[k][l0:l1] = r[k][lead:]
            if len(pr):
                out["quantiles"][:, l0:l1] = r["quantiles"][:, lead:]
        sd = np.sqrt(out["m2"] / (S - 1)) if S > 1 else np.full(L, np.nan)
        res = {"levels": labels, "count": out["count"], "weight": out["weight"], "mean": out["mean"], "sd": sd, "probs": pr,
               "quantiles": out["quantiles"], "p_above": out["p_above"], "draws": S}
        if return_draws:
            avg = out["draws"]                                                        # [L, pooled draws], chain after chain
            res["average"] = avg if combine_chains else avg.reshape(L, len(self.samplers), -1).transpose(0, 2, 1)
        return res

    # ------------------------------------------------------------------ describe_posterior
    @staticmethod
    def hdi_draws(ci, draws: int) -> int:
        """The draws m of the window that holds the mass ``ci`` of ``draws`` pooled draws: ceil(ci x draws) in exact rational arithmetic on the
        decimal text of ``ci`` (in floating point 0.7 x 10 is 7.000000000000001 and would give 8), clamped to [1, draws]."""
        c, m = ceil_fraction(ci, draws)
        if not 0 < c <= 1:
            raise ValueError(f"'ci' must hold masses in (0, 1], not {ci!r}")
        return max(1, min(int(draws), m))

    def describe_posterior(self, x_bart=None, x_bart0=None, X=None, X0=None, groups: Optional[Sequence[GroupTerm]] = None,
                           groups0: Optional[Sequence[GroupTerm]] = None, offset=None, offset0=None, treatment=None, levels=(1.0, 0.0),
                           type: str = "ev", ci=(0.95,), thresholds=(), rope=None, probs=(0.025, 0.5, 0.975), mad_constant: float = 1.0,
                           sample_new_levels: bool = True, seed: Optional[int] = None):
        """Per-row description of the posterior — what ``bayestestR::describe_posterior`` reports for every row of ``predict``'s matrix or of
        ``predict_contrast``'s effects — formed on the device without a [rows x draws] matrix, pooled over the chains in ONE call
        (``s4b_predict_describe``: the first chain's sampler with the others as its peers).  Any arm-0 argument (suffix 0) or ``treatment`` makes
        it the contrast of two arms, formed as ``predict_contrast`` forms it; otherwise the one arm's expected value as ``predict_quantiles`` forms
        it.  ``ci``: up to 8 masses in (0, 1]; the highest-density interval of a mass is the shortest window of m = ``hdi_draws(mass, draws)`` of
        the sorted draws (the lowest on a tie).  ``thresholds``: values whose exceedance is asked for; ``rope`` None or (low, high), the region of
        practical equivalence.  Every share is formed from the integer counts with one division.  Returns ``median``, ``mad`` (times
        ``mad_constant``; 1.4826 gives R's ``mad``), ``ci``, ``hdi`` [masses, 2, rows], ``hdi_draws`` [masses], ``hdi_start`` [masses, rows],
        ``probs`` and ``quantiles`` [Q, rows], ``thresholds`` with ``p_above`` and ``p_below`` [thresholds, rows] (both strict), ``pd`` (the
        probability of direction, max(P(> 0), P(< 0))), with a ROPE ``rope_share`` (the share of the draws inside [low, high]) and
        ``rope_share_hdi`` [masses, rows] (the share of the interval's draws inside it), and ``draws``."""
        if type == "ppd":
            raise ValueError("describe_posterior does not form 'ppd': its noise is drawn per element of the draws matrix (use predict)")
        if type not in ("ev", "indiv.bart"):
            raise ValueError("'type' must be one of ev, indiv.bart (indiv.fixef and indiv.ranef need no trees: use predict)")
        if not self.samplers:
            raise ValueError("describe_posterior requires 'bart_args' to contain 'keepTrees' as True")
        if x_bart is None:
            raise ValueError("describe_posterior needs x_bart, the new rows of the BART predictors")
        pr = np.atleast_1d(np.asarray(probs, dtype=np.float64))
        if pr.ndim != 1 or len(pr) > 16 or not np.all((pr >= 0.0) & (pr <= 1.0)):
            raise ValueError(f"'probs' must be a vector of at most 16 values in [0, 1], not {probs!r}")
        masses = [float(c) for c in np.atleast_1d(np.asarray(ci, dtype=np.float64))]
        if len(masses) > DESCRIBE_HDI_MAX:
            raise ValueError(f"'ci' holds {len(masses)} masses: at most {DESCRIBE_HDI_MAX} per call")
        thr = np.atleast_1d(np.asarray(thresholds, dtype=np.float64))
        if thr.ndim != 1 or np.any(np.isnan(thr)):
            raise ValueError(f"'thresholds' must be a vector without NaN, not {thresholds!r}")
        if rope is not None:
            rope = tuple(float(v) for v in rope)
            if len(rope) != 2 or not rope[0] <= rope[1]:
                raise ValueError(f"'rope' must be None or (low, high) with low <= high, not {rope!r}")
        T = len(thr)
        internal = np.r_[thr, 0.0, rope if rope is not None else ()]          # the call's thresholds, then 0 and the ends of the ROPE
        if len(internal) > DESCRIBE_THRESHOLDS_MAX:
            raise ValueError(f"'thresholds' holds {T} values: at most {DESCRIBE_THRESHOLDS_MAX - (3 if rope is not None else 1)} per call beside the binding's own")
        two = treatment is not None or any(a is not None for a in (x_bart0, X0, groups0, offset0))
        x_bart, x_bart0, kw, peer_kw = self._contrast_arms(x_bart, x_bart0, X, X0, groups, groups0, offset, offset0, treatment, levels, type,
                                                           sample_new_levels, seed)
        first = self.samplers[0]
        S = first.describe_draws() + sum(p.describe_draws() for p in peer_kw["peers"])
        m = np.array([self.hdi_draws(c, S) for c in masses], dtype=np.int32)
        r = first.predict_describe(x_bart, x_bart0, n_arms=2 if two else 1, hdi_count=m, thresholds=internal, probs=pr, **peer_kw, **kw)
        na, nb = r["n_above"].astype(np.int64), r["n_below"].astype(np.int64)
        res = {"median": r["median"], "mad": r["mad"] * float(mad_constant), "ci": np.asarray(masses), "hdi": r["hdi"], "hdi_draws": m.astype(np.int64),
               "hdi_start": r["hdi_start"], "probs": pr, "quantiles": r["quantiles"], "thresholds": thr, "p_above": na[:T] / S, "p_below": nb[:T] / S,
               "pd": np.maximum(na[T], nb[T]) / S, "draws": S}
        if rope is not None:
            first_in, end_in = nb[T + 1], S - na[T + 2]                      # the sorted draws [first_in, end_in) lie in [low, high]
            res["rope"] = rope
            res["rope_share"] = (S - nb[T + 1] - na[T + 2]) / S
            if len(m):
                start = r["hdi_start"].astype(np.int64)
                overlap = np.minimum(start + m[:, None], end_in[None, :]) - np.maximum(start, first_in[None, :])
                res["rope_share_hdi"] = np.maximum(overlap, 0) / m[:, None].astype(np.int64)
            else:
                res["rope_share_hdi"] = np.zeros((0, len(na[T])))
        return res

    # ------------------------------------------------------------------ predict_sorted
    def predict_sorted(self, x_bart=None, x_bart0=None, X=None, X0=None, groups: Optional[Sequence[GroupTerm]] = None,
                       groups0: Optional[Sequence[GroupTerm]] = None, offset=None, offset0=None, treatment=None, levels=(1.0, 0.0),
                       row_probs=(0.1, 0.25, 0.5, 0.75, 0.9), top=(0.1,), bottom=(0.1,), probs=(0.025, 0.5, 0.975), return_draws: bool = False,
                       type: str = "ev", sample_new_levels: bool = True, seed: Optional[int] = None):
        """Sorted effects: the distribution of the rows' values ACROSS THE ROWS within a posterior draw — its quantiles at ``row_probs``, each with
        a posterior band — and for every row the posterior probability of belonging to the most and the least affected group.  Any arm-0 argument
        (suffix 0) or ``treatment`` makes the values the contrast of two arms as ``predict_contrast`` forms it, otherwise the one arm's expected
        value as ``predict_quantiles`` forms it.  On the device without a [rows x draws] matrix and in ONE pooled call (``s4b_predict_sorted``: the
        first chain's sampler with the others as its peers).  ``top`` / ``bottom``: fractions f in (0, 1); the group of a draw is its
        m = ceil(f x rows) rows with the largest / smallest values (exact rational arithmetic on the decimal text of f, m < rows; with ties at
        the boundary fewer rows lie strictly beyond it).  Returns ``row_probs`` and ``sorted``, ``top`` / ``bottom`` (the fractions),
        ``top_count`` / ``bottom_count`` (m), ``cut_rank`` and ``cut`` (the per-draw boundary values: a row is in the top group of a draw when it
        lies strictly above the cut), each of ``sorted`` and ``cut`` a dict of ``mean``, ``sd`` (over the draws, ddof 1), ``quantiles`` [Q,
        statistics] and with ``return_draws`` ``draws`` [statistics, draws] chain after chain; ``p_top`` [top, rows] and ``p_bottom``
        [bottom, rows]; the raw int32 counts ``n_above`` and ``n_below`` [cuts, rows]; ``probs``, ``draws`` (the pooled count) and ``info``."""
        if type == "ppd":
            raise ValueError("predict_sorted does not form 'ppd': its noise is drawn per element of the draws matrix (use predict)")
        if type not in ("ev", "indiv.bart"):
            raise ValueError("'type' must be one of ev, indiv.bart (indiv.fixef and indiv.ranef need no trees: use predict)")
        if not self.samplers:
            raise ValueError("predict_sorted requires 'bart_args' to contain 'keepTrees' as True")
        if x_bart is None:
            raise ValueError("predict_sorted needs x_bart, the new rows of the BART predictors")
        pr = np.atleast_1d(np.asarray(probs, dtype=np.float64))
        if pr.ndim != 1 or len(pr) > 16 or not np.all((pr >= 0.0) & (pr <= 1.0)):
            raise ValueError(f"'probs' must be a vector of at most 16 values in [0, 1], not {probs!r}")
        rp = np.atleast_1d(np.asarray(row_probs, dtype=np.float64))
        if rp.ndim != 1 or len(rp) > SORTED_PROBS_MAX or not np.all((rp >= 0.0) & (rp <= 1.0)):
            raise ValueError(f"'row_probs' must be a vector of at most {SORTED_PROBS_MAX} values in [0, 1], not {row_probs!r}")
        tf = [float(f) for f in np.atleast_1d(np.asarray(top, dtype=np.float64))]
        bf = [float(f) for f in np.atleast_1d(np.asarray(bottom, dtype=np.float64))]
        if len(tf) + len(bf) > SORTED_CUTS_MAX:
            raise ValueError(f"'top' and 'bottom' hold {len(tf) + len(bf)} fractions together: at most {SORTED_CUTS_MAX} per call")
        rows = np.shape(x_bart)[0]
        for f in tf + bf:
            fraction_count(f, rows)          # (refused here, before the arms are formed)
        two = treatment is not None or any(a is not None for a in (x_bart0, X0, groups0, offset0))
        x_bart, x_bart0, kw, peer_kw = self._contrast_arms(x_bart, x_bart0, X, X0, groups, groups0, offset, offset0, treatment, levels, type,
                                                           sample_new_levels, seed)
        r = self.samplers[0].predict_sorted(x_bart, x_bart0, n_arms=2 if two else 1, row_probs=rp, top=tf, bottom=bf, probs=pr, **peer_kw, **kw)
        S, Qr = r["draws_pooled"], len(rp)
        L = Qr + len(tf) + len(bf)

        def part(rows_of):
            if L == 0:
                return None
            m2 = r["m2"][rows_of]
            out = {"mean": r["mean"][rows_of], "sd": np.sqrt(m2 / (S - 1)) if S > 1 else np.full(len(m2), np.nan),
                   "quantiles": r["quantiles"][:, rows_of] if r["quantiles"] is not None else np.zeros((0, len(m2)))}
            if return_draws:
                out["draws"] = r["draws"][rows_of]
            return out
        return {"row_probs": rp, "sorted": part(slice(0, Qr)), "top": np.asarray(tf), "bottom": np.asarray(bf), "top_count": r["top_count"],
                "bottom_count": r["bottom_count"], "cut_rank": r["cut_rank"], "cut": part(slice(Qr, L)), "p_top": r["p_top"], "p_bottom": r["p_bottom"],
                "n_above": r["n_above"], "n_below": r["n_below"], "probs": pr, "draws": S, "info": r["info"]}

    # ------------------------------------------------------------------ predict_projection
    def predict_projection(self, design, x_bart=None, x_bart0=None, X=None, X0=None, groups: Optional[Sequence[GroupTerm]] = None,
                           groups0: Optional[Sequence[GroupTerm]] = None, offset=None, offset0=None, treatment=None, levels=(1.0, 0.0),
                           row_weights=None, names=None, intercept: bool = True, center: bool = True, probs=(0.025, 0.5, 0.975), threshold=0.0,
                           tol: float = 1e-10, type: str = "ev", sample_new_levels: bool = True, seed: Optional[int] = None):
        """Posterior summarisation: which covariates moderate the effect (or the fitted value), by how much, with an interval.  For every posterior
        draw the rows' values — any arm-0 argument (suffix 0) or ``treatment`` makes them the contrast of two arms as ``predict_contrast`` forms it,
        otherwise the one arm's expected value as ``predict_quantiles`` forms it — are projected on ``design`` [rows x columns] by weighted least
        squares, on the device without a [rows x draws] matrix, in ONE pooled call (``s4b_predict_projection``: the first chain's sampler with the
        others as its peers).  ``intercept`` prepends a column of ones; ``center`` (with an intercept) subtracts from every other column its
        weighted mean, returned as ``center``: the slopes are unchanged, the intercept then IS the weighted average value or effect, and the normal
        equations are better conditioned.  At most 32 columns, the intercept included.  ``row_weights`` None (1) or [rows], non-negative.  The
        rank rule acts on the normal equations: a pivot of their Cholesky factorisation not above ``tol`` times its diagonal entry makes the design
        ``deficient`` and every result NaN.  Returns ``names``, ``coef`` [K, draws] (chain after chain), ``mean``, ``sd`` (ddof 1), ``probs``,
        ``quantiles`` [Q, K] and ``p_above`` [K] (the share of the draws strictly above ``threshold``) per coefficient, ``r2`` [draws] with
        ``r2_mean`` and ``r2_quantiles`` [Q] (the share of the weighted variation of the rows' values the projection captures, per draw),
        ``center`` [K], ``weight``, ``deficient``, ``draws`` and ``info``."""
        if type == "ppd":
            raise ValueError("predict_projection does not form 'ppd': its noise is drawn per element of the draws matrix (use predict)")
        if type not in ("ev", "indiv.bart"):
            raise ValueError("'type' must be one of ev, indiv.bart (indiv.fixef and indiv.ranef need no trees: use predict)")
        if not self.samplers:
            raise ValueError("predict_projection requires 'bart_args' to contain 'keepTrees' as True")
        if x_bart is None:
            raise ValueError("predict_projection needs x_bart, the new rows of the BART predictors")
        pr = np.atleast_1d(np.asarray(probs, dtype=np.float64))
        if pr.ndim != 1 or len(pr) > 16 or not np.all((pr >= 0.0) & (pr <= 1.0)):
            raise ValueError(f"'probs' must be a vector of at most 16 values in [0, 1], not {probs!r}")
        if threshold is not None and np.isnan(float(threshold)):
            raise ValueError("'threshold' is a NaN")
        if not 0.0 <= float(tol) < 1.0:
            raise ValueError(f"'tol' must lie in [0, 1), not {tol!r}")
        rows = np.shape(x_bart)[0]
        A = np.asarray(design, dtype=np.float64)
        if A.ndim == 1:
            A = A[:, None]
        if A.ndim != 2 or A.shape[0] != rows:
            raise ValueError(f"'design' must hold one row per row of x_bart ({rows}), not shape {A.shape}")
        if not np.all(np.isfinite(A)):
            raise ValueError("'design' holds a value that is not finite")
        cols = A.shape[1]
        K = cols + int(bool(intercept))
        if not 1 <= K <= PROJECTION_COLUMNS_MAX:
            raise ValueError(f"between 1 and {PROJECTION_COLUMNS_MAX} design columns, the intercept included, not {K}")
        if K > rows:
            raise ValueError(f"{K} design columns, the intercept included, but only {rows} rows")
        if names is None:
            names = [f"x{j + 1}" for j in range(cols)]
        names = [str(s) for s in names]
        if len(names) != cols:
            raise ValueError(f"'names' must name the {cols} columns of 'design', not {len(names)}")
        w = None
        if row_weights is not None:
            w = np.asarray(row_weights, dtype=np.float64)
            if w.shape != (rows,) or not np.all(np.isfinite(w)) or np.any(w < 0.0):
                raise ValueError(f"row_weights must be [{rows}] finite non-negative values")
        shift = np.zeros(K)
        if intercept:
            if center and cols:
                tot = float(rows) if w is None else float(w.sum())
                if tot > 0.0:
                    shift[1:] = (A.sum(axis=0) if w is None else w @ A) / tot
            A = np.column_stack([np.ones(rows), A - shift[1:]])
            names = ["(Intercept)"] + names
        two = treatment is not None or any(a is not None for a in (x_bart0, X0, groups0, offset0))
        x_bart, x_bart0, kw, peer_kw = self._contrast_arms(x_bart, x_bart0, X, X0, groups, groups0, offset, offset0, treatment, levels, type,
                                                           sample_new_levels, seed)
        r = self.samplers[0].predict_projection(x_test=x_bart, design=A, x_test0=x_bart0, n_arms=2 if two else 1, threshold=threshold, probs=pr, tol=tol,
                                                weights=w, **peer_kw, **kw)
        S = r["draws_pooled"]
        sd = np.sqrt(r["m2"][:K] / (S - 1)) if S > 1 else np.full(K, np.nan)
        q = r["quantiles"] if r["quantiles"] is not None else np.zeros((0, K + 1))
        return {"names": names, "coef": r["coef"], "mean": r["mean"][:K], "sd": sd, "probs": pr, "quantiles": q[:, :K],
                "p_above": None if r["p_above"] is None else r["p_above"][:K], "r2": r["r2"], "r2_mean": float(r["mean"][K]), "r2_quantiles": q[:, K],
                "center": shift, "weight": r["weight"], "deficient": r["deficient"], "draws": S, "info": r["info"]}

    # ------------------------------------------------------------------ predict_spread
    def predict_spread(self, x_bart=None, x_bart0=None, X=None, X0=None, groups: Optional[Sequence[GroupTerm]] = None,
                       groups0: Optional[Sequence[GroupTerm]] = None, offset=None, offset0=None, treatment=None, levels=(1.0, 0.0),
                       thresholds=(0.0,), row_weights=None, probs=(0.025, 0.5, 0.975), return_draws: bool = False, type: str = "ev",
                       sample_new_levels: bool = True, seed: Optional[int] = None):
        """Effect heterogeneity: how the rows' values are spread ACROSS THE ROWS within a posterior draw, and the posterior of that spread.  Any
        arm-0 argument (suffix 0) or ``treatment`` makes the values the contrast of two arms as ``predict_contrast`` forms it, otherwise the one
        arm's expected value as ``predict_quantiles`` forms it.  Per draw, on the device without a [rows x draws] matrix and in ONE pooled call
        (``s4b_predict_spread``: the first chain's sampler with the others as its peers): the weighted mean, the standard deviation over the rows
        (population form), the smallest and largest value, and for each of the up to 64 strictly ascending ``thresholds`` the share of the weight
        on the rows strictly above it and the part of the mean those rows contribute.  ``row_weights`` None (1) or [rows], non-negative, not all 0.
        Returns ``names`` (the 4 + 2 T statistics), per statistic ``mean``, ``sd`` (over the draws, ddof 1) and ``quantiles`` [Q, statistics],
        ``probs``, ``weight``, ``thresholds``, ``draws`` (the pooled count), ``info`` and the named views ``effect_sd``, ``share_above`` [T],
        ``part_above`` [T], ``mean_above`` [T] (part / share: the mean value among the rows above) and ``gain`` [T] (part - threshold x share: the
        gain of treating exactly the rows above at that cost), the last two NaN in a draw whose share is 0.  With ``return_draws`` a view is its
        draw vector ([draws] or [T, draws], chain after chain) and ``matrix`` [statistics, draws] is returned too; otherwise a view is the dict of
        its ``mean``, ``sd`` and ``quantiles`` over the draws."""
        if type == "ppd":
            raise ValueError("predict_spread does not form 'ppd': its noise is drawn per element of the draws matrix (use predict)")
        if type not in ("ev", "indiv.bart"):
            raise ValueError("'type' must be one of ev, indiv.bart (indiv.fixef and indiv.ranef need no trees: use predict)")
        if not self.samplers:
            raise ValueError("predict_spread requires 'bart_args' to contain 'keepTrees' as True")
        if x_bart is None:
            raise ValueError("predict_spread needs x_bart, the new rows of the BART predictors")
        pr = np.atleast_1d(np.asarray(probs, dtype=np.float64))
        if pr.ndim != 1 or len(pr) > 16 or not np.all((pr >= 0.0) & (pr <= 1.0)):
            raise ValueError(f"'probs' must be a vector of at most 16 values in [0, 1], not {probs!r}")
        th = np.atleast_1d(np.asarray(thresholds, dtype=np.float64))
        if th.ndim != 1 or len(th) > SPREAD_THRESHOLDS_MAX:
            raise ValueError(f"'thresholds' must be a vector of at most {SPREAD_THRESHOLDS_MAX} values, not {len(th) if th.ndim == 1 else th.shape}")
        if np.any(np.isnan(th)):
            raise ValueError("'thresholds' holds a NaN")
        if not np.all(th[1:] > th[:-1]):
            raise ValueError("'thresholds' must be strictly ascending")
        rows = np.shape(x_bart)[0]
        w = None
        if row_weights is not None:
            w = np.asarray(row_weights, dtype=np.float64)
            if w.shape != (rows,) or not np.all(np.isfinite(w)) or np.any(w < 0.0):
                raise ValueError(f"row_weights must be [{rows}] finite non-negative values")
            if not w.sum() > 0.0:
                raise ValueError("row_weights sum to 0: no row carries weight")
        two = treatment is not None or any(a is not None for a in (x_bart0, X0, groups0, offset0))
        x_bart, x_bart0, kw, peer_kw = self._contrast_arms(x_bart, x_bart0, X, X0, groups, groups0, offset, offset0, treatment, levels, type,
                                                           sample_new_levels, seed)
        r = self.samplers[0].predict_spread(x_test=x_bart, thresholds=th, x_test0=x_bart0, n_arms=2 if two else 1, probs=pr, weights=w,
                                            outputs=("mean", "m2", "draws"), **peer_kw, **kw)
        S, T, D = r["draws_pooled"], len(th), r["draws"]
        M = 4 + 2 * T
        sd = np.sqrt(r["m2"] / (S - 1)) if S > 1 else np.full(M, np.nan)
        q = r["quantiles"] if r["quantiles"] is not None else np.zeros((0, M))
        share, part = D[4:4 + T], D[4 + T:]
        with np.errstate(divide="ignore", invalid="ignore"):
            none = share == 0.0
            mean_above = np.where(none, np.nan, part / share)
            gain = np.where(none, np.nan, part - th[:, None] * share)

        def view(rows_of, derived=None):
            """A named view: the draws, or the summary over them (the device's for a statistic of the matrix, numpy's for a derived one)."""
            if return_draws:
                return D[rows_of] if derived is None else derived
            if derived is None:
                return {"mean": r["mean"][rows_of], "sd": sd[rows_of], "quantiles": q[:, rows_of]}
            with np.errstate(invalid="ignore"):
                return {"mean": derived.mean(axis=1), "sd": derived.std(axis=1, ddof=1) if S > 1 else np.full(len(derived), np.nan),
                        "quantiles": np.quantile(derived, pr, axis=1) if len(pr) else np.zeros((0, len(derived)))}
        res = {"names": r["names"], "mean": r["mean"], "sd": sd, "probs": pr, "quantiles": q, "weight": r["weight"], "thresholds": th, "draws": S,
               "info": r["info"], "effect_sd": view(1), "share_above": view(slice(4, 4 + T)), "part_above": view(slice(4 + T, M)),
               "mean_above": view(None, mean_above), "gain": view(None, gain)}
        if return_draws:
            res["matrix"] = D
        return res

    def bayes_R2(self, x_bart=None, X=None, groups: Optional[Sequence[GroupTerm]] = None, offset=None, probs=(0.025, 0.5, 0.975),
                 sample_new_levels: bool = True, seed: Optional[int] = None):
        """The Bayes R-squared of Gelman, Goodrich, Gabry and Vehtari (rstanarm's ``bayes_R2``) at the given rows, for a continuous response: per
        posterior draw ``R2 = v / (v + sigma^2)`` with ``v`` the variance of the fitted values across the rows (R's ``var``: n - 1 in the
        denominator) and ``sigma`` the draw's residual standard deviation.  The variance comes from ONE ``predict_spread`` call with one arm, so
        no [rows x draws] matrix is formed.  Returns ``r2`` [draws] (chain after chain), ``mean``, ``median``, ``probs`` and ``quantiles``."""
        if self.family == "binomial":
            raise ValueError("bayes_R2 is defined here for a continuous response only: a binary fit has no residual standard deviation")
        pr = np.atleast_1d(np.asarray(probs, dtype=np.float64))
        if pr.ndim != 1 or not np.all((pr >= 0.0) & (pr <= 1.0)):
            raise ValueError(f"'probs' must be a vector of values in [0, 1], not {probs!r}")
        if x_bart is None:
            raise ValueError("bayes_R2 needs x_bart, the rows of the BART predictors")
        n = np.shape(x_bart)[0]
        if n < 2:
            raise ValueError("bayes_R2 needs at least two rows")
        s = self.predict_spread(x_bart=x_bart, X=X, groups=groups, offset=offset, thresholds=(), probs=(), return_draws=True, type="ev",
                                sample_new_levels=sample_new_levels, seed=seed)
        sig = self.stan[self.par_names.index("aux.1")]               # [iter, chain]; pooled draw k is draw k % iter of chain k // iter
        r2 = self.r2_from_spread(s["effect_sd"], sig.T.reshape(-1), n)
        return {"r2": r2, "mean": float(r2.mean()), "median": float(np.median(r2)), "probs": pr, "quantiles": np.quantile(r2, pr) if len(pr) else np.zeros(0)}

    @staticmethod
    def r2_from_spread(sd_rows, sigma, n: int):
        """``v / (v + sigma^2)`` per draw, ``v = sd_rows^2 n / (n - 1)``: the population-form standard deviation across the ``n`` rows, as
        ``predict_spread`` returns it, turned into R's ``var``."""
        sd_rows, sigma = np.asarray(sd_rows, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
        if sd_rows.shape != sigma.shape:
            raise ValueError(f"{sd_rows.shape[0] if sd_rows.ndim else 1} draws of the spread, but {sigma.shape[0] if sigma.ndim else 1} of sigma")
        v = sd_rows * sd_rows * (float(n) / float(n - 1))
        return v / (v + sigma * sigma)

    # ------------------------------------------------------------------ predict_ppd
    def predict_ppd(self, x_bart=None, X=None, groups: Optional[Sequence[GroupTerm]] = None, offset=None, y=None, probs=(0.025, 0.5, 0.975),
                    obs_weights=None, sample_new_levels: bool = True, seed: Optional[int] = None):
        """The posterior predictive distribution at new rows, read out on the device without ``predict(type="ppd")``'s [rows x draws] matrix, in ONE
        pooled call (``s4b_predict_ppd``: the first chain's sampler with the others as its peers).  Continuous response: ``quantiles`` [Q, rows],
        the ``probs`` quantiles (R's type 7) of ``y_rep = ev + sigma sqrt(1 / obs_weights) e`` — prediction intervals for new observations —
        with sigma each chain's ``aux.1`` draws and ``e`` a counter-based standard normal, a pure function of (``noise_key``, row, pooled draw).
        ``noise_key`` comes from ``seed`` (None: fresh entropy) and is returned, with the ``seed`` that reproduces the whole call.  Binary response:
        no replicate is formed (a row's predictive distribution is Bernoulli(mean of ev): ``predict_summary``); ``probs`` must be empty.
        With held-out responses ``y`` [rows] the call scores them per row: ``lpd`` (log mean_k p(y | theta_k)), ``p_waic`` (var_k log p, ddof 1),
        ``elpd_waic = lpd - p_waic``, ``pit`` (continuous only), and over the rows ``elpd_waic_total``, its ``se = sqrt(rows var(elpd_waic))``
        (ddof 1) and, with two or more probs, ``coverage``: the share of ``y`` inside the outermost pair of requested quantiles.
        Needs bart_args keepTrees."""
        if not self.samplers:
            raise ValueError("predict_ppd requires 'bart_args' to contain 'keepTrees' as True")
        if x_bart is None:
            raise ValueError("predict_ppd needs x_bart, the new rows of the BART predictors")
        binary = self.family == "binomial"
        pr = np.atleast_1d(np.asarray(probs, dtype=np.float64))
        if pr.ndim != 1 or len(pr) > 16 or not np.all((pr >= 0.0) & (pr <= 1.0)):
            raise ValueError(f"'probs' must be a vector of at most 16 values in [0, 1], not {probs!r}")
        if binary and len(pr):
            raise ValueError("predict_ppd forms no quantiles for a binary response: a row's predictive distribution is Bernoulli(mean of ev), which "
                             "predict_summary gives (pass probs=())")
        if not len(pr) and y is None:
            raise ValueError("predict_ppd: nothing asked for (no probs, no y)")
        x_bart = np.asarray(x_bart, dtype=np.float64)
        rows = x_bart.shape[0]
        if y is not None:
            y = np.asarray(y, dtype=np.float64)
            if y.shape != (rows,):
                raise ValueError(f"y must have shape [{rows}], not {y.shape}")
        row_scale = None
        if obs_weights is not None:
            w = np.asarray(obs_weights, dtype=np.float64)
            if w.shape != (rows,) or not np.all(np.isfinite(w) & (w > 0.0)):
                raise ValueError(f"obs_weights must be {rows} finite values > 0")
            row_scale = 1.0 / np.sqrt(w)                             # reference R/generics.R:452-459: sd = sigma sqrt(1 / w)
        ss = np.random.SeedSequence(seed)                            # (default_rng(seed) is default_rng(SeedSequence(seed)): predict's draws of unseen levels)
        noise_key = int(ss.generate_state(1, np.uint64)[0])
        linear = self._summary_linear("ev", X, groups, offset, sample_new_levels, np.random.default_rng(ss))
        first, others = linear(0), [linear(c) for c in range(1, len(self.samplers))]
        sig = self.stan[self.par_names.index("aux.1")]               # [iter, chain]
        r = self.samplers[0].predict_ppd(x_bart, pr, y=y, sigma=None if binary else sig[:, 0], row_scale=row_scale, noise_key=noise_key,
                                         peers=self.samplers[1:], peer_sigma=None if binary else [sig[:, c] for c in range(1, len(self.samplers))],
                                         peer_dense_coef=None if first["dense"] is None else [a["dense_coef"] for a in others],
                                         peer_ell_coef=None if first["ell_index"] is None else [a["ell_coef"] for a in others], **first)
        S = r["draws"]
        out = {"probs": pr, "quantiles": r["quantiles"], "draws": S, "noise_key": noise_key, "seed": ss.entropy}
        if y is not None:
            p_waic = r["lm2"] / (S - 1) if S > 1 else np.full(rows, np.nan)
            elpd = r["lpd"] - p_waic
            out.update(lpd=r["lpd"], p_waic=p_waic, elpd_waic=elpd, elpd_waic_total=float(elpd.sum()),
                       se=float(np.sqrt(rows * np.var(elpd, ddof=1))) if rows > 1 else float("nan"))
            if not binary:
                out["pit"] = r["pit"]
            if len(pr) >= 2:
                lo, hi = r["quantiles"][int(np.argmin(pr))], r["quantiles"][int(np.argmax(pr))]
                out["coverage"] = float(np.mean((y >= lo) & (y <= hi)))
        return out

    # ------------------------------------------------------------------ pp_check
    def pp_check(self, x_bart=None, X=None, groups: Optional[Sequence[GroupTerm]] = None, y=None, thresholds=(), row_weights=None, obs_weights=None,
                 probs=(0.025, 0.5, 0.975), seed: Optional[int] = None, return_draws: bool = False, offset=None, sample_new_levels: bool = True):
        """Posterior predictive checks (rstanarm's ``pp_check``): do data replicated from the fitted model look like the observed ``y`` [rows]?  Per
        posterior draw the replicate ``y_rep`` is formed on the device — continuous response: ``ev + sigma sqrt(1 / obs_weights) e``, the very
        replicate ``predict_ppd`` summarises under the same ``seed``; binary response: Bernoulli(ev) — and reduced ACROSS THE ROWS without ever
        being stored, in ONE pooled call (``s4b_predict_check``: the first chain's sampler with the others as its peers).  The statistics are the
        weighted (``row_weights``: None or [rows], non-negative, not all 0) ``mean``, ``sd``, ``skewness``, ``min``, ``max``, ``share_above`` [T]
        (the share of the weight strictly above each of the up to 64 ascending ``thresholds``; none for a binary response) and ``discrepancy``
        (continuous: the chi^2 of Gelman, Meng and Stern; binary: the deviance).  Each view is a dict of ``observed`` (the statistic of ``y``), ``mean``,
        ``sd`` (ddof 1) and ``quantiles`` [Q] over the draws and ``p_value``, the share of draws whose replicated statistic is >= the observed one
        (``discrepancy``: the share with disc_rep >= disc_obs; its ``observed`` is the mean of disc_obs over the draws); with ``return_draws`` also
        ``draws`` (``discrepancy``: ``draws`` and ``draws_obs``), chain after chain, and ``matrix`` [7 + T, draws] is returned.  Also ``names``,
        ``probs``, ``thresholds``, ``weight``, ``draws`` (the pooled count), ``info``, ``noise_key`` and the ``seed`` that reproduces the whole
        call.  Needs bart_args keepTrees."""
        if not self.samplers:
            raise ValueError("pp_check requires 'bart_args' to contain 'keepTrees' as True")
        if x_bart is None:
            raise ValueError("pp_check needs x_bart, the rows of the BART predictors")
        if y is None:
            raise ValueError("pp_check needs y, the observed responses at the rows")
        binary = self.family == "binomial"
        pr = np.atleast_1d(np.asarray(probs, dtype=np.float64))
        if pr.ndim != 1 or len(pr) > 16 or not np.all((pr >= 0.0) & (pr <= 1.0)):
            raise ValueError(f"'probs' must be a vector of at most 16 values in [0, 1], not {probs!r}")
        th = np.atleast_1d(np.asarray(thresholds, dtype=np.float64))
        if th.ndim != 1 or len(th) > SPREAD_THRESHOLDS_MAX:
            raise ValueError(f"'thresholds' must be a vector of at most {SPREAD_THRESHOLDS_MAX} values, not {len(th) if th.ndim == 1 else th.shape}")
        if np.any(np.isnan(th)) or not np.all(th[1:] > th[:-1]):
            raise ValueError("'thresholds' must be strictly ascending and hold no NaN")
        if binary and len(th):
            raise ValueError("pp_check takes no thresholds for a binary response: a replicate is 0 or 1, its mean is the share of ones")
        x_bart = np.asarray(x_bart, dtype=np.float64)
        rows = x_bart.shape[0]
        y = np.asarray(y, dtype=np.float64)
        if y.shape != (rows,) or not np.all(np.isfinite(y)):
            raise ValueError(f"y must be {rows} finite values")
        if binary and not np.all((y == 0.0) | (y == 1.0)):
            raise ValueError("y must be 0 or 1 for a binary response")
        w = None
        if row_weights is not None:
            w = np.asarray(row_weights, dtype=np.float64)
            if w.shape != (rows,) or not np.all(np.isfinite(w)) or np.any(w < 0.0):
                raise ValueError(f"row_weights must be [{rows}] finite non-negative values")
            if not w.sum() > 0.0:
                raise ValueError("row_weights sum to 0: no row carries weight")
        row_scale = None
        if obs_weights is not None:
            ow = np.asarray(obs_weights, dtype=np.float64)
            if ow.shape != (rows,) or not np.all(np.isfinite(ow) & (ow > 0.0)):
                raise ValueError(f"obs_weights must be {rows} finite values > 0")
            row_scale = 1.0 / np.sqrt(ow)                            # reference R/generics.R:452-459: sd = sigma sqrt(1 / w)
        ss = np.random.SeedSequence(seed)                            # (predict_ppd's handling: the same seed gives the same noise_key)
        noise_key = int(ss.generate_state(1, np.uint64)[0])
        linear = self._summary_linear("ev", X, groups, offset, sample_new_levels, np.random.default_rng(ss))
        first, others = linear(0), [linear(c) for c in range(1, len(self.samplers))]
        sig = self.stan[self.par_names.index("aux.1")]               # [iter, chain]
        r = self.samplers[0].predict_check(x_bart, y=y, thresholds=th, probs=pr, sigma=None if binary else sig[:, 0], row_scale=row_scale,
                                           noise_key=noise_key, weights=w, peers=self.samplers[1:],
                                           peer_sigma=None if binary else [sig[:, c] for c in range(1, len(self.samplers))],
                                           peer_dense_coef=None if first["dense"] is None else [a["dense_coef"] for a in others],
                                           peer_ell_coef=None if first["ell_index"] is None else [a["ell_coef"] for a in others], **first)
        S, T, D, obs = r["draws_pooled"], len(th), r["draws"], r["observed"]
        M = 7 + T
        sd = np.sqrt(r["m2"] / (S - 1)) if S > 1 else np.full(M, np.nan)
        q = r["quantiles"] if r["quantiles"] is not None else np.zeros((0, M))

        def summary(v):
            return {"mean": float(v.mean()), "sd": float(v.std(ddof=1)) if S > 1 else float("nan"),
                    "quantiles": np.quantile(v, pr) if len(pr) else np.zeros(0)}

        def view(m):
            """A statistic of the matrix: the device's summary over the draws, the host's statistic of y, the p-value from the draws."""
            out = {"observed": float(obs[m]), "mean": float(r["mean"][m]), "sd": float(sd[m]), "quantiles": q[:, m], "p_value": float(np.mean(D[m] >= obs[m]))}
            if return_draws:
                out["draws"] = D[m]
            return out
        with np.errstate(divide="ignore", invalid="ignore"):
            skew = np.where(D[1] > 0.0, D[2] / (D[1] * D[1] * D[1]), np.nan)
            skew_obs = float(obs[2] / obs[1] ** 3) if obs[1] > 0.0 else float("nan")
            skewness = dict(summary(skew) if not np.any(np.isnan(skew)) else {"mean": float("nan"), "sd": float("nan"), "quantiles": np.full(len(pr), np.nan)},
                            observed=skew_obs, p_value=float(np.mean(skew >= skew_obs)))
        disc = dict(summary(D[5 + T]), observed=float(D[6 + T].mean()), p_value=float(np.mean(D[5 + T] >= D[6 + T])))
        if return_draws:
            skewness["draws"] = skew
            disc.update(draws=D[5 + T], draws_obs=D[6 + T])
        res = {"names": r["names"], "probs": pr, "thresholds": th, "weight": r["weight"], "draws": S, "info": r["info"], "noise_key": noise_key,
               "seed": ss.entropy, "mean": view(0), "sd": view(1), "skewness": skewness, "min": view(3), "max": view(4),
               "share_above": [view(5 + j) for j in range(T)], "discrepancy": disc}
        if return_draws:
            res["matrix"] = D
        return res

    # ------------------------------------------------------------------ predict_loo
    def predict_loo(self, x_bart=None, X=None, groups: Optional[Sequence[GroupTerm]] = None, offset=None, y=None, obs_weights=None, r_eff: float = 1.0,
                    sample_new_levels: bool = True, seed: Optional[int] = None):
        """PSIS-LOO (``loo::loo()`` on the log-likelihood matrix) of the responses ``y`` [rows] at the rows, read out on the device without the
        [rows x draws] matrix, in ONE pooled call (``s4b_predict_loo``: the first chain's sampler with the others as its peers).  The likelihood is
        ``predict_ppd``'s: normal with sd = sigma sqrt(1 / obs_weights), or Bernoulli-probit.  A scalar ``r_eff`` in (0, 1] sets the tail length
        ``ceil(min(S / 5, 3 sqrt(S / r_eff)))`` (at most 1024).  Per row: ``elpd_loo``, ``pareto_k`` (+inf where no tail was fitted), ``lpd``,
        ``p_loo = lpd - elpd_loo``, ``ess``; over the rows ``elpd_loo_total``, ``p_loo_total``, ``se = sqrt(rows var(elpd_loo))`` (ddof 1),
        ``k_threshold = min(1 - 1 / log10(S), 0.7)``, ``n_high_k`` (rows above it), ``draws`` and ``tail_len``.  Restated from the published
        algorithm, not pinned against the R package.  Needs bart_args keepTrees."""
        if not self.samplers:
            raise ValueError("predict_loo requires 'bart_args' to contain 'keepTrees' as True")
        if x_bart is None:
            raise ValueError("predict_loo needs x_bart, the rows of the BART predictors")
        if y is None:
            raise ValueError("predict_loo needs y, the responses of the rows")
        x_bart = np.asarray(x_bart, dtype=np.float64)
        rows = x_bart.shape[0]
        y = np.asarray(y, dtype=np.float64)
        if y.shape != (rows,):
            raise ValueError(f"y must have shape [{rows}], not {y.shape}")
        if not (np.ndim(r_eff) == 0 and 0.0 < float(r_eff) <= 1.0):
            raise ValueError(f"'r_eff' must be one value in (0, 1], not {r_eff!r}")
        binary = self.family == "binomial"
        row_scale = None
        if obs_weights is not None:
            w = np.asarray(obs_weights, dtype=np.float64)
            if w.shape != (rows,) or not np.all(np.isfinite(w) & (w > 0.0)):
                raise ValueError(f"obs_weights must be {rows} finite values > 0")
            row_scale = 1.0 / np.sqrt(w)                             # reference R/generics.R:452-459: sd = sigma sqrt(1 / w)
        sig = self.stan[self.par_names.index("aux.1")]               # [iter, chain]
        S = sig.shape[0] * len(self.samplers)
        tail_len = 0                                                 # r_eff = 1: the library's own integer rule
        if float(r_eff) != 1.0:
            tail_len = int(np.ceil(min(S / 5.0, 3.0 * np.sqrt(S / float(r_eff)))))
            if tail_len > 1024:
                raise ValueError(f"r_eff = {r_eff!r} asks for a tail of {tail_len} of the {S} draws: at most 1024")
            if tail_len < 5:                                         # (20 draws or fewer: no tail is fitted under any r_eff, the default says the same)
                tail_len = 0
        linear = self._summary_linear("ev", X, groups, offset, sample_new_levels, np.random.default_rng(seed))
        first, others = linear(0), [linear(c) for c in range(1, len(self.samplers))]
        r = self.samplers[0].predict_loo(x_bart, y=y, sigma=None if binary else sig[:, 0], row_scale=row_scale, tail_len=tail_len,
                                         peers=self.samplers[1:], peer_sigma=None if binary else [sig[:, c] for c in range(1, len(self.samplers))],
                                         peer_dense_coef=None if first["dense"] is None else [a["dense_coef"] for a in others],
                                         peer_ell_coef=None if first["ell_index"] is None else [a["ell_coef"] for a in others], **first)
        S = r["draws"]
        p_loo = r["lpd"] - r["elpd_loo"]
        thr = min(1.0 - 1.0 / np.log10(S), 0.7) if S > 1 else float("-inf")
        return {"elpd_loo": r["elpd_loo"], "pareto_k": r["pareto_k"], "lpd": r["lpd"], "p_loo": p_loo, "ess": r["ess"],
                "elpd_loo_total": float(r["elpd_loo"].sum()), "p_loo_total": float(p_loo.sum()),
                "se": float(np.sqrt(rows * np.var(r["elpd_loo"], ddof=1))) if rows > 1 else float("nan"),
                "k_threshold": float(thr), "n_high_k": int(np.sum(r["pareto_k"] > thr)), "draws": S, "tail_len": r["tail_len"]}

    # ------------------------------------------------------------------ predict_convergence
    def predict_convergence(self, x_bart=None, X=None, groups: Optional[Sequence[GroupTerm]] = None, offset=None, type: str = "ev", quantity: str = "ev",
                            y=None, obs_weights=None, split: bool = True, rhat_threshold: float = 1.01, sample_new_levels: bool = True,
                            seed: Optional[int] = None):
        """``Rhat`` and ``n_eff`` for every row: split R-hat and the effective sample size (Stan's estimators) of the rows' draws with the chains
        kept apart, read out on the device without the [rows x draws] matrix, in ONE pooled call (``s4b_predict_convergence``: the first chain's
        sampler with the others as its peers, every chain cut to the shortest and, with ``split``, halved).  ``quantity`` "ev": the series is
        ``predict_summary``'s value (``type`` "ev" or "indiv.bart"); "lik": the likelihood of the responses ``y`` [rows] as ``predict_loo`` forms
        it (sd = sigma sqrt(1 / obs_weights), or Bernoulli-probit) — the series of ``loo::relative_eff``.  Per row: ``rhat``, ``ess``, ``mean``,
        ``mcse`` (the Monte-Carlo standard error of ``mean``), ``n_pairs`` (autocorrelation pairs Geyer's sequence kept); NaN / -1 where a row has
        no answer (fewer than 4 draws per chain, a value that is not finite, every chain constant).  Over the rows: ``rhat_max``, ``n_high_rhat``
        (rows above ``rhat_threshold``), ``ess_min``; ``chains``, ``chain_len``, ``draws`` (chains x chain_len, the draws used).  "lik" adds
        ``r_eff = ess / draws`` per row.  Needs bart_args keepTrees."""
        if quantity not in ("ev", "lik"):
            raise ValueError(f"'quantity' must be one of ev, lik, not {quantity!r}")
        if type == "ppd":
            raise ValueError("predict_convergence does not form 'ppd': its noise is drawn per element of the draws matrix (use predict)")
        if type not in ("ev", "indiv.bart"):
            raise ValueError("'type' must be one of ev, indiv.bart (indiv.fixef and indiv.ranef need no trees: use predict)")
        if quantity == "lik" and type != "ev":
            raise ValueError("quantity 'lik' is the likelihood of y under the whole prediction: 'type' must be ev")
        if not self.samplers:
            raise ValueError("predict_convergence requires 'bart_args' to contain 'keepTrees' as True")
        if x_bart is None:
            raise ValueError("predict_convergence needs x_bart, the rows of the BART predictors")
        if quantity == "lik" and y is None:
            raise ValueError("predict_convergence: quantity 'lik' needs y, the responses of the rows")
        if quantity == "ev" and y is not None:
            raise ValueError("predict_convergence: quantity 'ev' takes no y (quantity 'lik' is the likelihood of y)")
        if quantity == "ev" and obs_weights is not None:
            raise ValueError("predict_convergence: quantity 'ev' takes no obs_weights")
        if not (np.ndim(rhat_threshold) == 0 and float(rhat_threshold) >= 1.0):
            raise ValueError(f"'rhat_threshold' must be one value >= 1, not {rhat_threshold!r}")
        x_bart = np.asarray(x_bart, dtype=np.float64)
        rows = x_bart.shape[0]
        lik = quantity == "lik"
        binary = self.family == "binomial"
        row_scale = None
        if lik:
            y = np.asarray(y, dtype=np.float64)
            if y.shape != (rows,):
                raise ValueError(f"y must have shape [{rows}], not {y.shape}")
            if obs_weights is not None:
                w = np.asarray(obs_weights, dtype=np.float64)
                if w.shape != (rows,) or not np.all(np.isfinite(w) & (w > 0.0)):
                    raise ValueError(f"obs_weights must be {rows} finite values > 0")
                row_scale = 1.0 / np.sqrt(w)                         # reference R/generics.R:452-459: sd = sigma sqrt(1 / w)
        need_sigma = lik and not binary
        sig = self.stan[self.par_names.index("aux.1")] if need_sigma else None          # [iter, chain]
        linear = self._summary_linear(type, X, groups, offset, sample_new_levels, np.random.default_rng(seed))
        first, others = linear(0), [linear(c) for c in range(1, len(self.samplers))]
        r = self.samplers[0].predict_convergence(x_bart, quantity=quantity, split=bool(split), y=y if lik else None,
                                                 sigma=sig[:, 0] if need_sigma else None, row_scale=row_scale, peers=self.samplers[1:],
                                                 peer_sigma=[sig[:, c] for c in range(1, len(self.samplers))] if need_sigma else None,
                                                 peer_dense_coef=None if first["dense"] is None else [a["dense_coef"] for a in others],
                                                 peer_ell_coef=None if first["ell_index"] is None else [a["ell_coef"] for a in others], **first)
        used = r["chains"] * r["chain_len"]
        with np.errstate(invalid="ignore"):
            high = int(np.sum(r["rhat"] > float(rhat_threshold)))
        fin_r, fin_e = r["rhat"][np.isfinite(r["rhat"])], r["ess"][np.isfinite(r["ess"])]
        out = {"rhat": r["rhat"], "ess": r["ess"], "mean": r["mean"], "mcse": r["mcse"], "n_pairs": r["n_pairs"],
               "rhat_max": float(fin_r.max()) if len(fin_r) else float("nan"), "n_high_rhat": high,
               "ess_min": float(fin_e.min()) if len(fin_e) else float("nan"), "chains": r["chains"], "chain_len": r["chain_len"], "draws": used}
        if lik:
            out["r_eff"] = r["ess"] / used if used else np.full(rows, np.nan)
        return out

    def export_bart_states(self) -> list:
        """``stan4bart_exportBARTState`` per chain (reference R/stan4bart_fit.R:572-580): byte strings that
        ``attach_stored_samplers`` turns back into predict-capable samplers, in this or another process."""
        if not self.samplers:
            raise ValueError("exporting the BART state requires bart_args keepTrees")
        return [s.export_bart_state() for s in self.samplers]

    def attach_stored_samplers(self, states: Sequence[bytes], lib=None, prefix: str = "s4b_", device: int = 0):
        """``stan4bart_createStoredBARTSampler`` for every chain: afterwards ``predict`` works without the fitting samplers."""
        from .abi import StoredSampler
        if lib is None:
            from ._lib import load_library
            lib = load_library()
        self.close()
        self.samplers = [StoredSampler(lib, prefix, st, device) for st in states]

    def close(self):
        for s in self.samplers:
            s.free()
        self.samplers = []


def _stack(chain_results, phase, key, sub=None):
    arrs = []
    for r in chain_results:
        a = r[phase][key] if sub is None else r[phase][key][sub]
        arrs.append(np.asarray(a))
    return np.stack(arrs, axis=-1)


class _BatchGroup:
    """The sweep group of one thread batch of stan4bart(batch_chains=True): made by the first chain that joins (its library and device),
    left by every chain on its way out, freed after the batch."""

    def __init__(self, size: int):
        import threading
        self.size, self.group, self.lock = size, None, threading.Lock()

    def join(self, s, device: int):
        from .abi import SweepGroup
        with self.lock:
            if self.group is None:
                self.group = SweepGroup(s._lib, s._pfx, device, self.size)
            self.group.join(s)

    def leave(self, s):
        with self.lock:
            if self.group is not None:
                self.group.leave(s)

    def close(self, total: Optional[dict]) -> Optional[dict]:
        with self.lock:
            if self.group is None:
                return total
            st = self.group.stats()
            self.group.free()
            self.group = None
        if total is None:
            return st
        return {k: total[k] + st[k] for k in st}


def stan4bart(y, x_bart, X=None, groups: Sequence[GroupTerm] = (), x_bart_test=None, X_test=None,
              groups_test: Optional[Sequence[GroupTerm]] = None, offset=None, offset_test=None, offset_type: str = "default",
              family: str = "gaussian", chains: int = 4, seed: Optional[int] = None, iter: int = 2000, warmup: int = 1000,
              keep_warmup: bool = True, make_sampler: Optional[Callable] = None, treatment=None, callback: Optional[Callable] = None,
              cores: int = 1, batch_chains: bool = False, **kw) -> Stan4bartFit:
    """The reference's ``stan4bart()`` after its formula front end (R/stan4bart.R:1-297 -> arrays): runs ``chains``
    chains with the single-threaded seeding rule (R/stan4bart_fit.R:545-554) and packages the draws
    (``package_samples``, R/stan4bart.R:299-455).  With ``bart_args = {"keepTrees": True}`` the samplers stay alive
    inside the fit (``object$sampler.bart``) so that ``predict`` can use the kept trees; call ``close()`` when done.

    ``treatment = ("X" | "x_bart", column)`` names a binary treatment column: the test sample becomes the training rows
    with the treatment flipped, i.e. the counterfactual (reference R/stan4bart.R:93-120, tests/testthat/test-10-treatment.R).
    ``callback(yhat_train, yhat_test, stan_pars, par_names)`` is evaluated after every iteration inside the sampler
    (reference src/init.cpp:849-911, tests/testthat/test-11-callback.R); its results come back as ``extract("callback")``.

    ``cores > 1`` runs the chains concurrently with the reference's parallel seeding rule (R/stan4bart_fit.R:515-533: worker c
    does ``set.seed(sample.int(.Machine$integer.max, chains)[c])``), here as host threads sharing the device: one chain leaves
    most of an MI355X idle at n = 1e6, four interleaved chains finish about twice as fast as four in a row.

    ``batch_chains=True`` (needs ``cores > 1``) puts each thread batch of chains into one sweep group: while a chain's tree sweep runs
    on one workgroup (n <= 4 096), the sweeps of the batch's chains go out as one launch, one workgroup per chain.  The draws are
    those of ``batch_chains=False``; ``fit.batch_stats`` counts the batched launches and the sweeps that went out on their own."""
    if batch_chains and cores <= 1:
        raise ValueError("batch_chains=True batches the sweeps of chains run concurrently: it needs cores > 1")
    make_sampler = make_sampler or hip_sampler_factory()
    if treatment is not None:
        if x_bart_test is not None or X_test is not None:
            raise ValueError("'treatment' builds the test sample itself: do not pass test data as well")
        where, col = treatment
        if where not in ("X", "x_bart"):
            raise ValueError("treatment must be ('X', column) or ('x_bart', column)")
        src = np.asarray(X if where == "X" else x_bart, dtype=np.float64)
        vals = np.unique(src[:, col])
        if len(vals) != 2:
            raise ValueError("treatment must be binary")
        flipped = src.copy()
        flipped[:, col] = np.where(src[:, col] == vals[0], vals[1], vals[0])
        x_bart_test = flipped if where == "x_bart" else np.asarray(x_bart, dtype=np.float64)
        X_test = flipped if where == "X" else (None if X is None else np.asarray(X, dtype=np.float64))
        groups_test = list(groups) if len(groups) else None
        offset_test = offset
    names_box: list = []
    cb = None
    if callback is not None:
        cb = lambda tr, te, sp: np.asarray(callback(tr, te, sp, names_box[0]), dtype=np.float64)
    import os
    rng = RRng(seed if seed is not None else int.from_bytes(os.urandom(4), "little") % INT_MAX)
    keep_trees = bool((kw.get("bart_args") or {}).get("keepTrees", False))
    results, samplers = [None] * chains, [None] * chains
    args_box = [None]

    def one_chain(c, chain_rng, sharing=1, group=None):
        args = make_sampler_args(y, x_bart, X=X, groups=groups, x_test=x_bart_test, family=family, iter=iter, warmup=warmup,
                                 offset=offset, offset_type=offset_type, keep_fits=True, callback=cb, **kw)
        args_box[0] = args
        args.seed = int(chain_rng.sample_int(INT_MAX, 1)[0])
        s = make_sampler(args, chain_rng.state)
        r = {}
        try:
            if group is not None:
                group.join(s, args.device)
            if sharing > 1 and hasattr(s, "set_device_sharing"):
                s.set_device_sharing(sharing)                 # host threads that share the GPU while this chain runs (its batch)
            names_box[:] = [s.stan_par_names()]
            if warmup > 0:
                r["warmup"] = s.run(warmup, True, 0)
            s.disengage_adaptation()
            r["sample"] = s.run(iter - warmup, False, 0)
            r["par_names"] = s.stan_par_names()
            qr_back_transform(args, r)       # stan_args = {"QR": True}: beta rows back to the design's scale (R/stan4bart_fit.R:560-570)
            r["range.bart"] = s.get_bart_data_range()
            chain_rng.state = s.get_r_rng_state()
            if group is not None:
                group.leave(s)
        except Exception:
            if group is not None:
                group.leave(s)
            s.free()
            raise
        if keep_trees:
            samplers[c] = s
        else:
            s.free()
        results[c] = r

    batch_stats = None
    if cores <= 1 or chains == 1:
        try:
            for c in range(chains):        # one stream continued from chain to chain (R/stan4bart_fit.R:545-554)
                one_chain(c, rng)
        except Exception:                  # a later chain failed: the kept samplers of the earlier ones hold device memory
            for sm in samplers:
                if sm is not None:
                    sm.free()
            raise
    else:
        import threading
        seeds = chain_seeds(int(rng.sample_int(INT_MAX, 1)[0]) if seed is None else seed, chains)
        errors = []

        def guarded(c, sharing, group):
            try:
                one_chain(c, RRng(int(seeds[c])), sharing, group)
            except Exception as e:   # surfaced after the join
                errors.append(e)
        pending = list(range(chains))
        while pending:
            batch, pending = pending[:cores], pending[cores:]
            group = _BatchGroup(len(batch)) if batch_chains else None
            try:
                th = [threading.Thread(target=guarded, args=(c, len(batch), group)) for c in batch]
                [t.start() for t in th]
                [t.join() for t in th]
            finally:
                if group is not None:
                    batch_stats = group.close(batch_stats)
        if errors:
            for sm in samplers:
                if sm is not None:
                    sm.free()
            raise errors[0]
    samplers = [sm for sm in samplers if sm is not None]
    args = args_box[0]

    def pack(phase):
        return dict(stan=_stack(results, phase, "stan"), bart_train=_stack(results, phase, "bart", "train"),
                    bart_test=_stack(results, phase, "bart", "test") if x_bart_test is not None else None,
                    bart_varcount=_stack(results, phase, "bart", "varcount"),
                    k=_stack(results, phase, "bart", "k") if "k" in results[0][phase]["bart"] else None,     # (R/stan4bart.R:389-399)
                    callback=(np.stack([np.stack(r[phase]["callback"], axis=1) for r in results], axis=2)
                              if callback is not None else None))
    smp = pack("sample")
    n = len(y)
    Xa = np.zeros((n, 0)) if X is None else np.asarray(X, dtype=np.float64).reshape(n, -1)
    terms = args.extras["group_terms"]
    terms_test = None
    if groups_test is not None and len(groups_test):
        by = {g.name: g for g in groups_test}
        terms_test = [by[g.name] for g in terms]
    return Stan4bartFit(
        family=family, par_names=results[0]["par_names"], stan=smp["stan"], bart_train=smp["bart_train"], bart_test=smp["bart_test"],
        bart_varcount=smp["bart_varcount"], warmup=pack("warmup") if (warmup > 0 and keep_warmup) else None,
        X=Xa, X_means=np.asarray(args.extras["xbar"]), X_test=None if X_test is None else np.asarray(X_test, dtype=np.float64),
        terms=terms, terms_test=terms_test, offset=None if offset is None else np.asarray(offset, dtype=np.float64),
        offset_test=None if offset_test is None else np.asarray(offset_test, dtype=np.float64), offset_type=offset_type,
        range_bart=np.stack([r["range.bart"] for r in results], axis=1), samplers=samplers, callback=smp["callback"],
        weights=None if kw.get("weights") is None else np.asarray(kw["weights"], dtype=np.float64), k=smp["k"], batch_stats=batch_stats,
        latents=args.latents)
