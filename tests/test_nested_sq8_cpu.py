"""The certificate of the nested search's int8 first pass, on the CPU.

For an accepted row r of family p(r): lb(r) ≤ score(r) ≤ ub(r).  LBp = the family's largest lb over the rows that
hold a real certificate, T = the k-th largest LBp (nothing when fewer than k families have one).  A row is
re-scored exactly iff it has a record, ub ≥ T and ub ≥ LBp of its family; the nested top k of the re-scored rows
alone must be the exhaustive one.

  * the argument: on small random corpora and on adversarial intervals, the rule reproduces the exhaustive
    result (docs and scores, ties by doc);
  * the bound on the input: with `oracle/bounds_reference.py`'s float64 restatement of the int8 interval, unit
    rows in families of the GPU test's sizes leave at most 10 % of 4,097 rows to re-score at k = 10.
"""
import numpy as np
import pytest

from oracle import bounds_reference as BR

FAMILY_SIZES = (1, 2, 3, 5, 17, 64, 65, 300)
NONE = -np.inf            # "no LBp" / "no floor": below every score and every bound


def families(n, rng, sizes=FAMILY_SIZES):
    """(parent id, doc) per row: families of sizes drawn from `sizes`, each followed by its parent doc."""
    pid, doc, p, d, left = [], [], 0, 0, n
    while left > 0:
        f = min(int(rng.choice(sizes)), left)
        pid += [p] * f
        doc += list(range(d, d + f))
        d += f + 1
        p += 1
        left -= f
    return np.asarray(pid), np.asarray(doc)


def nested_topk(score, pid, doc, k, rows):
    """The k best families among `rows` (a mask): per family the row with (max score, then min doc), those by
    (score desc, doc asc).  A NaN score is never a hit."""
    keep = rows & ~np.isnan(score)
    s, p, d = score[keep], pid[keep], doc[keep]
    order = np.lexsort((d, -s))
    s, p, d = s[order], p[order], d[order]
    _, first = np.unique(p, return_index=True)
    first.sort()
    return d[first][:k].tolist(), s[first][:k].tolist()


def floor_and_lbp(lb, cert, record, pid, k):
    n_par = int(pid.max()) + 1
    lbp = np.full(n_par, NONE)
    real = cert & record
    np.maximum.at(lbp, pid[real], lb[real])
    have = np.sort(lbp[lbp > NONE])[::-1]
    return (have[k - 1] if len(have) >= k else NONE), lbp


def settled_rows(lb, ub, cert, record, pid, k, strict=False, floor_rank=0):
    """The rule.  cert: the row holds a real certificate (else its ub counts as +inf and its lb as nothing).
    strict / floor_rank: the two arithmetic mutations the tests must catch."""
    T, lbp = floor_and_lbp(lb, cert, record, pid, k + floor_rank)
    u = np.where(cert, ub, np.inf)
    own = u > lbp[pid] if strict else u >= lbp[pid]
    return record & (u >= T) & own


def check(score, lb, ub, cert, record, pid, doc, k):
    with np.errstate(invalid="ignore"):
        assert np.all(~cert | ~record | ((lb <= score) & (score <= ub)))
    want = nested_topk(score, pid, doc, k, record)
    got = nested_topk(score, pid, doc, k, settled_rows(lb, ub, cert, record, pid, k))
    assert got == want, (k, got, want)
    return want


# ------------------------------------------------------------------------------------------------
# the argument
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(40))
def test_rule_equals_exhaustive_on_random_intervals(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 400))
    pid, doc = families(n, rng, sizes=(1, 2, 3, 5, 17))
    levels = int(rng.choice([3, 16, 10 ** 6]))                 # few distinct scores: ties everywhere
    score = rng.integers(0, levels, n) / levels
    w = rng.random(n) * rng.choice([0.0, 0.02, 0.3])           # zero width: lb = score = ub
    lb, ub = score - w * rng.random(n), score + w * rng.random(n)
    record = rng.random(n) < rng.choice([1.0, 0.5, 0.05])      # a filter
    cert = rng.random(n) < rng.choice([1.0, 0.9, 0.0])         # rows without a real certificate...
    score = np.where(~cert & (rng.random(n) < 0.5), np.nan, score)   # ...half of them score NaN
    for k in (1, 2, 10, 64):
        check(score, lb, ub, cert, record, pid, doc, k)


@pytest.mark.parametrize("sim", [BR.EUCLIDEAN, BR.DOT_PRODUCT, BR.COSINE, BR.MAXIMUM_INNER_PRODUCT])
def test_rule_equals_exhaustive_on_reference_intervals(sim):
    """Intervals of the int8 inequality itself and exact float64 scores of small random corpora."""
    rng = np.random.default_rng(100 + sim)
    for dim, n in ((7, 300), (96, 500)):
        x = rng.standard_normal((n, dim)).astype(np.float32)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        x[::50] = x[1]                                          # duplicates across families
        q = rng.standard_normal((3, dim)).astype(np.float32)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        pid, doc = families(n, rng, sizes=(1, 2, 3, 5, 17))
        R, Q = BR.Quantised(x), BR.Quantised(q)
        lo, hi, _, _ = BR.full_interval(sim, R, Q, dim)
        raw = Q.x @ R.x.T if sim != BR.EUCLIDEAN else ((Q.x[:, None, :] - R.x[None, :, :]) ** 2).sum(-1)
        for i in range(3):
            lb, ub = BR.score_image(sim, lo[i], hi[i], Q.x2[i], R.x2)
            score = BR.score64(sim, raw[i], Q.x2[i], R.x2)
            all_rows = np.ones(n, bool)
            for k in (1, 10, 64):
                check(score, lb, ub, all_rows, all_rows, pid, doc, k)


def test_adversarial_intervals():
    one = lambda *v: np.asarray(v, float)                      # noqa: E731
    # a best child whose lb lies below a sibling's: family 0 = {A: 0.9 in [0.5, 0.95], B: 0.8 in [0.78, 0.85]}
    score, lb, ub = one(0.9, 0.8, 0.7), one(0.5, 0.78, 0.6), one(0.95, 0.85, 0.75)
    pid, doc = np.array([0, 0, 1]), np.array([0, 1, 3])
    yes = np.ones(3, bool)
    assert check(score, lb, ub, yes, yes, pid, doc, 1) == ([0], [0.9])
    assert settled_rows(lb, ub, yes, yes, pid, 1).tolist() == [True, True, False]   # (C: ub 0.75 < T = 0.78)
    # equal scores across families at rank k, zero-width intervals: the lower doc takes the place
    score = one(0.9, 0.5, 0.5, 0.5, 0.1)
    pid, doc = np.array([0, 1, 2, 3, 4]), np.array([0, 2, 4, 6, 8])
    yes = np.ones(5, bool)
    assert check(score, score, score, yes, yes, pid, doc, 2) == ([0, 2], [0.9, 0.5])
    assert check(score, score, score, yes, yes, pid, doc, 3) == ([0, 2, 4], [0.9, 0.5, 0.5])
    # ...and with loose ones that overlap the floor from both sides
    assert check(score, score - one(0, 0.2, 0, 0.3, 0), score + one(0, 0, 0.2, 0.3, 0.39), yes, yes, pid, doc, 2) == \
        ([0, 2], [0.9, 0.5])
    # equal scores inside a family: every copy is settled, the lower doc wins
    score, pid, doc = one(0.5, 0.5, 0.4), np.array([0, 0, 1]), np.array([3, 5, 7])
    yes = np.ones(3, bool)
    assert check(score, score, score, yes, yes, pid, doc, 1) == ([3], [0.5])
    # T = nothing: fewer families with an LBp than k — a family of rows without a certificate is still found
    score, lb, ub = one(0.3, 0.2, 0.9, np.nan), one(0.25, 0.1, 0.0, 0.0), one(0.35, 0.3, np.inf, np.inf)
    pid, doc = np.array([0, 0, 1, 1]), np.array([0, 1, 3, 4])
    cert, yes = np.array([True, True, False, False]), np.ones(4, bool)
    assert check(score, lb, ub, cert, yes, pid, doc, 10) == ([3, 0], [0.9, 0.3])
    assert floor_and_lbp(lb, cert, yes, pid, 10)[0] == NONE
    # a row that is not accepted has no record and is never settled, whatever its bounds
    record = np.array([True, True, False, True])
    assert check(score, lb, ub, cert, record, pid, doc, 10) == ([0], [0.3])


def test_the_mutations_are_caught():
    """The checks above have teeth: dropping the equality of ub ≥ LBp loses a family whose interval has no width,
    and a floor taken one LBp too high (the (k − 1)-th) loses the k-th family.  (One taken too low only settles
    more rows; the GPU file's exact count of the settled rows catches that.)"""
    one = lambda *v: np.asarray(v, float)                      # noqa: E731
    score, pid, doc = one(0.5, 0.5, 0.4), np.array([0, 0, 1]), np.array([3, 5, 7])
    yes = np.ones(3, bool)
    strict = settled_rows(score, score, yes, yes, pid, 1, strict=True)
    assert nested_topk(score, pid, doc, 1, strict) != nested_topk(score, pid, doc, 1, yes)
    score, pid, doc = one(0.9, 0.8, 0.7), np.array([0, 1, 2]), np.array([0, 2, 4])
    early = settled_rows(score, score, yes, yes, pid, 2, floor_rank=-1)
    assert nested_topk(score, pid, doc, 2, early) != nested_topk(score, pid, doc, 2, yes)


# ------------------------------------------------------------------------------------------------
# the bound on the input: what the inequality alone leaves to re-score
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [7, 50, 96, 128, 768, 1000, 1030])
def test_unit_rows_leave_at_most_a_tenth_to_settle(dim):
    n, k = 4097, 10
    rng = np.random.default_rng(dim)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = rng.standard_normal((4, dim)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    pid, _ = families(n, np.random.default_rng(11))
    R, Q = BR.Quantised(x), BR.Quantised(q)
    yes = np.ones(n, bool)
    for sim in (BR.EUCLIDEAN, BR.DOT_PRODUCT, BR.COSINE, BR.MAXIMUM_INNER_PRODUCT):
        lo, hi, _, _ = BR.full_interval(sim, R, Q, dim)
        for i in range(4):
            lb, ub = BR.score_image(sim, lo[i], hi[i], Q.x2[i], R.x2)
            settled = int(settled_rows(lb, ub, yes, yes, pid, k).sum())
            print(f"dim {dim} sim {sim} query {i}: {settled} of {n} rows to settle at k = {k}")
            assert k <= settled <= 0.10 * n, (dim, sim, i, settled)
