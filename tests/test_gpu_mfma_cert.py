"""The bf16×3 batched path's candidates and certificate, looked at directly (osk_mfma.hip, batched_search).

tests/test_gpu_batched.py compares final top-10 lists, which notice a wrong certificate only when a true top-k
row sits outside the 16 candidates of its shard.  Here the path's intermediate records are read back (testing
build, osk_view_debug_copy) and held to oracle/mfma_reference.py and to the oracle's ORDER_DEVICE scores, on
the views of tests/mfma_inputs.py, k = 12, every similarity, dims with 4, 8, 24, 32 and 128 K-steps:

(a) split: "qsplit" is fragments(split(queries)) and "qnorm" the device-order |q|², bit for bit; the view's K-steps,
    error constant and per-shard largest |x|² are the reference's;
(b) error model, one-sided, no tolerance: every (query, row) of the visible view has its approximate score a in
    "akeys", and the oracle's score e satisfies e ≤ U(a) with the certificate's own U;
(c) candidates: "akeys" is the same with every tile on the full path, without quick tests, without the pilot and
    under another unit split; no candidate is a refused row, no accepted row is missing from a list that is not
    full, the pilot's 16th score does not exceed the final one, and the slot overflow happens; on a view whose
    15 best rows sit in the pilot tile and whose 16th sits in a later tile that keeps its survivors in slots, the
    candidates are the 16 best rows (a pilot threshold one place too high drops the 16th);
(d) flags: `rescore`'s certificate restated from "akeys", the oracle's scores and U equals "flags", and where a
    flag is 0 no row outside the candidates belongs in the shard's top k;
(e) end to end: docs, score bits and shards equal the oracle's, also on a view the int8 paths refuse (scales
    2^-70 … 2^63), on views whose |q|²·|x|² leaves float's range (components at 2^±32) and through near-tie
    clusters, which only the exact fallback can order;
(f) tightness, recorded: the largest (e − a)/(U(a) − a) and the share of plain `O.synth` queries that fell back
    (OSK_MFMA_TIGHTNESS_OUT names the JSON file; profiles/mfma_cert/tightness.json holds one MI355X run).
"""
import contextlib
import json
import os

import numpy as np
import pytest

import mfma_inputs as MI
from opensearch_amd import _lib, lucene as LU
from oracle import bounds_reference as BR
from oracle import mfma_reference as MR

pytestmark = pytest.mark.gpu

SIMS = [LU.VectorSimilarityFunction(s) for s in range(4)]
K, KC = MI.K, MI.KC
TUNE_DEFAULTS = {"mfma_min_batch": 96, "sq8_cost_pct": 100, "mfma_ablate": 0, "mfma_units": 0}
ABLATIONS = {"full path": 8, "no quick tests": 32, "no pilot": 16}
UNITS = (4, 10)          # 28 tiles of the tiled view in units of 7 and of 3 tiles: both |x|² parity slots in use
TIGHTNESS = {}


@contextlib.contextmanager
def tuned(**kv):
    try:
        for k, v in kv.items():
            _lib.tune(k, v)
        yield
    finally:
        for k in kv:
            _lib.tune(k, TUNE_DEFAULTS[k])


@contextlib.contextmanager
def opened(view, units=UNITS[0]):
    """The view on the testing build, batches ≥ 16 on the bf16×3 path whatever the cost model says."""
    with _lib.testing(), tuned(mfma_min_batch=16, sq8_cost_pct=100000, mfma_units=units):
        ds, readers = view.open(LU)
        try:
            yield ds
        finally:
            ds.close()
            for r in readers:
                r.close()


class Run:
    """One search of all the view's queries and the records it left."""

    def __init__(self, ds, view, filtered, ablate=0):
        nq, S = len(view.queries), view.n_shards
        with tuned(mfma_ablate=ablate):
            calls, self.full_before = ds.counter("mfma_calls"), ds.counter("mfma_full_tiles")
            self.fb_before = ds.counter("mfma_fallback_queries")
            self.out = ds.search(view.queries, K, 0, K, accept=view.accept if filtered else None)
            assert ds.counter("mfma_calls") == calls + 1, "the search did not take the bf16x3 path"
        self.full_tiles = ds.counter("mfma_full_tiles") - self.full_before
        self.fallbacks = ds.counter("mfma_fallback_queries") - self.fb_before
        copy = lambda name, n, dt: MI.BI.debug_copy(ds, name, n, dt)
        self.akeys = copy("akeys", nq * S * KC, np.uint64).reshape(nq, S, KC)
        self.acounts = copy("acounts", nq * S, np.int32).reshape(nq, S)
        self.flags = copy("flags", nq, np.int32)
        if not ablate & 16:
            self.pkeys = copy("pkeys", nq * S * KC, np.uint64).reshape(nq, S, KC)
            self.pcounts = copy("pcounts", nq * S, np.int32).reshape(nq, S)
        self.qnorm = copy("qnorm", nq, np.float32)
        self.maxnorm2 = copy("mfma_maxnorm2", S, np.float32)
        self.c = float(copy("mfma_c", 1, np.float64)[0])
        self.ks = int(copy("mfma_ks", 1, np.int64)[0])
        live = np.arange(KC)[None, None, :] < self.acounts[:, :, None]
        self.vrow = np.where(live, 0xFFFFFFFF - (self.akeys & 0xFFFFFFFF).astype(np.int64), -1)
        self.score = np.where(live, BR.from_sortable((self.akeys >> 32).astype(np.uint32)), np.float32(0.0)).astype(np.float32)
        assert not (self.akeys[~live] != 0).any() and (self.akeys[live] != 0).all(), "counts and keys disagree"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def views(sim, dim):
    return {"visible": MI.visible_view(sim, dim), "tiled": MI.tiled_view(sim, dim)}


# ---------------------------------------------------------------------------------------------------------
def check_split(sim, dim):
    """(a)"""
    for name, view in views(sim, dim).items():
        with opened(view) as ds:
            r = Run(ds, view, False)
            nq = len(view.queries)
            n_rb = (nq + 255) // 256 * 16
            assert r.ks == MR.ks_of(dim) and r.c == MR.c(r.ks)
            want = MR.fragments(MR.split(view.queries), r.ks, n_rb)
            got = MI.BI.debug_copy(ds, "qsplit", want.size, np.uint16).reshape(want.shape)
            assert np.array_equal(got, want), f"{name}: qsplit differs in {int((got != want).sum())} of {want.size} halves"
            assert np.array_equal(bits(r.qnorm), bits(view.qnorm)), f"{name}: |q|² differs from the device order's"
            assert np.array_equal(bits(r.maxnorm2), bits(view.shard_maxnorm2)), f"{name}: per-shard largest |x|²"


def visible_scores(view, r):
    """The approximate score of every (query, view row) out of "akeys": float32 [nq, n], NaN where a row is
    in no list."""
    nq = len(view.queries)
    a = np.full((nq, len(view.rows)), np.nan, np.float32)
    q = np.broadcast_to(np.arange(nq)[:, None, None], r.vrow.shape)
    have = r.vrow >= 0
    a[q[have], r.vrow[have]] = r.score[have]
    return a, have.sum()


def check_error_model(sim, dim):
    """(b) and (f).  Rows whose oracle score is NaN are exempt; a NaN or infinite approximate score counts as
    U = +inf."""
    view = MI.visible_view(sim, dim)
    with opened(view) as ds:
        r = Run(ds, view, False)
    e = view.scores
    a, n_have = visible_scores(view, r)
    missing = np.isnan(a) & ~np.isnan(e)
    assert not missing.any(), f"{int(missing.sum())} (query, row) pairs with an oracle score are in no candidate " \
        f"list, first {np.argwhere(missing)[0]}"
    sh = view.shard_of_row
    with np.errstate(all="ignore"):
        u = MR.U(int(sim), a.astype(np.float64), r.c, np.sqrt(r.maxnorm2.astype(np.float64))[sh][None, :],
                 np.sqrt(np.maximum(r.qnorm, np.float32(0.0)).astype(np.float64))[:, None])
        u = np.where(np.isfinite(a), u, np.inf)
        judged = ~np.isnan(e) & ~np.isnan(a)
        # (EUCLIDEAN: where U is clamped at score 1 the ratio says nothing about the bound; such pairs are left out)
        open_ = judged & np.isfinite(u) & (u > a) & ((int(sim) != MR.EUCLIDEAN) | (u < 1.0))
        used = np.where(open_, (e.astype(np.float64) - a) / (u - a), 0.0)
    ratio = float(np.max(used))
    fallback = record_tightness(sim, dim, ratio)
    print(f"bf16x3 tightness {sim.name} dim {dim}: largest (e - a)/(U - a) = {ratio:.4f}, synth fallback share {fallback:.3f}")
    bad = judged & ~(e <= u)
    if bad.any():
        q, x = np.argwhere(bad)[0]
        raise AssertionError(f"{int(bad.sum())} pairs with e > U(a); first: query {q} row {x} (shard {sh[x]}): "
                             f"e {e[q, x]!r} a {a[q, x]!r} U {u[q, x]!r}; largest (e - a)/(U - a) {ratio:.3f}")


def record_tightness(sim, dim, ratio):
    """(f) the share of the tiled view's plain `O.synth` queries (its rows: `O.synth` and the tame special rows)
    whose certificate failed, and the largest share of the error bound in use."""
    view = MI.tiled_view(sim, dim)
    with opened(view) as ds:
        r = Run(ds, view, False)
    plain = slice(3, 3 + MI.N_SYNTH_QUERIES_TILED)
    fallback = float((r.flags[plain] != 0).mean())
    TIGHTNESS[f"{sim.name}-{dim}"] = {"largest (e - a)/(U(a) - a), U not clamped at score 1": round(ratio, 5),
                                      "share of plain synth queries that fell back": round(fallback, 4)}
    out = os.environ.get("OSK_MFMA_TIGHTNESS_OUT")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(TIGHTNESS, f, indent=1, sort_keys=True)
    return fallback


def check_candidates(sim, dim):
    """(c).  Ablated runs skip the exact fallback: only their "akeys" are compared."""
    for name, view in views(sim, dim).items():
        accepted_in = lambda filtered: view.accepted if filtered else np.ones(len(view.rows), bool)
        base = {}
        with opened(view) as ds:
            for filtered in (False, True):
                r = base[filtered] = Run(ds, view, filtered)
                what = f"{name}, {'filtered' if filtered else 'unfiltered'}"
                acc = accepted_in(filtered)
                assert acc[r.vrow[r.vrow >= 0]].all(), what + ": a candidate the filter refuses"
                assert (r.akeys[:, :, :-1] >= r.akeys[:, :, 1:]).all(), what + ": a list out of order"
                # a list that is not full holds every accepted row of its shard that can be a hit
                hits = np.stack([(~np.isnan(view.scores[:, acc & (view.shard_of_row == s)])).sum(axis=1)
                                 for s in range(view.n_shards)], axis=1)
                short = r.acounts < KC
                assert (r.acounts[short] >= hits[short]).all(), what + ": a short list lost a row"
                both = r.pcounts >= KC
                assert (r.acounts[both] == KC).all()
                assert ((r.pkeys[:, :, KC - 1] >> 32)[both] <= (r.akeys[:, :, KC - 1] >> 32)[both]).all(), \
                    what + ": the pilot's 16th score exceeds the final 16th"
                for label, ablate in ABLATIONS.items():
                    o = Run(ds, view, filtered, ablate)
                    assert np.array_equal(o.akeys, r.akeys) and np.array_equal(o.acounts, r.acounts), \
                        f"{what}: akeys differ with {label} in {int((o.akeys != r.akeys).any(axis=2).sum())} lists"
                    if ablate == 8 and name == "visible":
                        # every tile on the full path offers every row: the descending sort of all rows' keys
                        per_shard = np.bincount(view.shard_of_row[acc], minlength=view.n_shards)
                        assert np.array_equal(o.acounts, np.broadcast_to(per_shard, o.acounts.shape)), \
                            what + ": a row of the visible view has no key"
                        for sh in range(view.n_shards):   # the lists hold exactly the shard's accepted rows
                            want = np.flatnonzero(acc & (view.shard_of_row == sh))
                            assert np.array_equal(np.sort(o.vrow[:, sh, :len(want)], axis=1),
                                                  np.broadcast_to(want, (len(view.queries), len(want)))), (what, sh)
            if name == "tiled":
                # query 0 equals 8 near-duplicate rows of one tile: more survivors than the tile's 4 slots
                assert base[False].full_tiles > 0, "no tile overflowed its survivor slots"
                assert (view.shard_of_row[MI.DUP_ROWS[0]] == 1) and \
                    np.isin(np.arange(MI.DUP_ROWS[0], sum(MI.DUP_ROWS)), base[False].vrow[MI.Q_DUP, 1]).all()
        with opened(view, UNITS[1]) as ds:
            for filtered in (False, True):
                o = Run(ds, view, filtered)
                assert np.array_equal(o.akeys, base[filtered].akeys), \
                    f"{name}: akeys differ between mfma_units {UNITS[0]} and {UNITS[1]}"
    check_pilot_threshold(sim, dim)


def check_pilot_threshold(sim, dim):
    """(c) on the pilot view: the pilot's threshold may drop no row of the final 16.  The 16th best row of every
    query sits in a tile that keeps its survivors in slots (one tile overflows: the pilot tile itself)."""
    view = MI.pilot_view(sim, dim)
    want = np.concatenate([np.arange(15), [MI.PILOT_LATE]])
    with opened(view, units=1) as ds:
        r = Run(ds, view, False)
        assert r.full_tiles == 1, f"{r.full_tiles} tiles took the full path, not the pilot tile alone"
        assert (r.pcounts == KC).all() and (r.acounts == KC).all()
        assert np.array_equal(r.vrow[:, 0, :], np.broadcast_to(want, (len(view.queries), KC))), \
            "the candidates are not the 16 best rows in order"
        for label, ablate in ABLATIONS.items():
            o = Run(ds, view, False, ablate)
            assert np.array_equal(o.akeys, r.akeys), f"pilot view: akeys differ with {label}"
        assert_results(view, r.out, False, "pilot view")


def check_flags(sim, dim):
    """(d)"""
    for name, view in views(sim, dim).items():
        with opened(view) as ds:
            runs = {filtered: Run(ds, view, filtered) for filtered in (False, True)}
        for filtered, r in runs.items():
            what = f"{name}, {'filtered' if filtered else 'unfiltered'}"
            fail, und, e_kth = view.restated_flags(r.score, r.vrow, r.acounts, r.c, r.maxnorm2, r.qnorm)
            assert und.mean() <= 0.01, f"{what}: {und.mean():.4f} of the certificates are too close to call"
            sure_fail = (fail & ~und).any(axis=1)
            sure_pass = ~(fail | und).any(axis=1)
            assert (r.flags[sure_fail] != 0).all(), \
                f"{what}: flag 0 where the certificate fails: queries {np.flatnonzero(sure_fail & (r.flags == 0))[:8]}"
            assert (r.flags[sure_pass] == 0).all(), \
                f"{what}: flag set where every certificate holds: queries {np.flatnonzero(sure_pass & (r.flags != 0))[:8]}"
            assert r.fallbacks == int((r.flags != 0).sum())
            if name == "tiled" and not filtered:   # the near-tie clusters cannot be certified
                assert r.flags[MI.Q_TIE0] != 0 and r.flags[MI.Q_TIE1] != 0
            # flag 0: no row outside the candidates beats or ties-with-a-lower-doc the shard's k-th hit
            acc = view.accepted if filtered else np.ones(len(view.rows), bool)
            S = view.scores
            for q in np.flatnonzero(r.flags == 0):
                for s in np.flatnonzero(r.acounts[q] == KC):
                    cand = r.vrow[q, s]
                    order = np.lexsort((view.doc_of_row[cand], -np.nan_to_num(S[q, cand].astype(np.float64), nan=-np.inf)))
                    kth = cand[order[K - 1]]
                    rest = np.flatnonzero(acc & (view.shard_of_row == s) & ~np.isnan(S[q]))
                    rest = rest[~np.isin(rest, cand)]
                    beats = (S[q, rest] > S[q, kth]) | ((S[q, rest] == S[q, kth]) & (view.doc_of_row[rest] < view.doc_of_row[kth]))
                    assert not beats.any(), f"{what}: query {q} shard {s} certified, yet row {rest[beats][0]} " \
                        f"(score {S[q, rest[beats][0]]!r}) belongs above the k-th hit {S[q, kth]!r}"


def assert_results(view, out, filtered, what, queries=None):
    s, d, sh, cnt, _, _ = out
    for j, (es, ed, esh) in enumerate(view.expected(filtered, queries)):
        qi = j if queries is None else queries[j]
        n = len(ed)
        assert cnt[j] == n, (what, qi, int(cnt[j]), n)
        assert np.array_equal(d[j, :n], ed) and np.array_equal(sh[j, :n], esh), (what, qi, d[j, :n], ed)
        assert np.array_equal(bits(s[j, :n]), bits(es)), (what, qi)


def check_end_to_end(sim, dim):
    """(e)"""
    all_views = dict(views(sim, dim), extreme=MI.extreme_view(sim, dim), pow32=MI.pow_view(sim, dim, 32),
                     pow_minus_32=MI.pow_view(sim, dim, -32))
    for name, view in all_views.items():
        with opened(view) as ds:
            for filtered in (False, True):
                r = Run(ds, view, filtered)
                assert_results(view, r.out, filtered, f"{name}, {'filtered' if filtered else 'unfiltered'}")
                if name == "tiled" and not filtered:
                    # near-tie clusters: right only through the fallback
                    assert r.flags[MI.Q_TIE0] != 0 and r.flags[MI.Q_TIE1] != 0 and r.fallbacks >= 2


CHECKS = {"split": check_split, "error_model": check_error_model, "candidates": check_candidates,
          "flags": check_flags, "end_to_end": check_end_to_end}
# the check varies fastest: a (similarity, dim)'s views and oracle scores are built once and kept
CASES = [pytest.param(s, d, c, id=f"{s.name}-{d}-{c}") for s in SIMS for d in MI.DIMS for c in CHECKS]


@pytest.mark.parametrize("sim,dim,check", CASES)
def test_mfma(sim, dim, check):
    CHECKS[check](sim, dim)
