"""Shared cases and the fp64 checker for ops.gbt_best_split (K10b), used by
test_gbt_cat_cpu.py (torch path) and test_gbt_cat_gpu.py (kernel).

The histograms are built directly, not through K10, so the inputs are
deterministic. Counts are small integers and the residual sums small integers
(or multiples of 1/8), so every partial sum is exact in fp32 and the only
rounding in the op is that of the gain's products, quotients and sums.

A case is a dict: cnt, s float32 [n, F, nb]; ftype int32 [F]; lam;
planted {node: (feature, threshold, mask)} for the nodes whose answer is
stated by hand (the runner-up's gain is far below the winner's there, or the
answer is a no-split)."""

import itertools
from pathlib import Path

import numpy as np
import torch

GOLDEN = Path(__file__).parent / "golden" / "gbt" / "sample_gbt_cat_32"

MIN_GAIN = 1e-12                 # build_tree's has_split constant
ULPS = 16 * 2.0 ** -23           # checker item 2: 16 fp32 roundings


def signed64(m: int) -> int:
    return m - (1 << 64) if m >= 1 << 63 else m


def unsigned64(m: int) -> int:
    return m & ((1 << 64) - 1)


# ------------------------------------------------------------------ builders

def _types(kind: str, F: int) -> torch.Tensor:
    if kind == "cont":
        t = [0] * F
    elif kind == "cat":
        t = [8] * F
    else:                        # mixed: odd features categorical
        t = [8 * (f % 2) for f in range(F)]
    return torch.tensor(t, dtype=torch.int32)


def random_case(n, F, nb, kind, lam, seed, max_cat=64):
    """Integer histograms: cnt in 0..5 with about a third of the bins empty,
    s in -8..8 where cnt > 0. Categories at or above max_cat stay empty."""
    g = torch.Generator().manual_seed(seed)
    cnt = torch.randint(0, 6, (n, F, nb), generator=g).float()
    cnt = cnt * (torch.rand(n, F, nb, generator=g) < 0.7)
    s = torch.randint(-8, 9, (n, F, nb), generator=g).float() * (cnt > 0)
    ftype = _types(kind, F)
    if nb > max_cat:
        cat = ftype != 0
        cnt[:, cat, max_cat:] = 0
        s[:, cat, max_cat:] = 0
    return dict(name=f"random n{n} F{F} nb{nb} {kind} lam{lam:g}", cnt=cnt,
                s=s, ftype=ftype, lam=float(lam), planted={})


SHAPES = list(itertools.product((1, 8), (1, 5, 8), (2, 3, 64)))
_KINDS = ("cont", "cat", "mixed")


def shape_cases():
    """Every (n_nodes, F, nb) of the issue's shape list, the feature kinds
    and lam in {0, 1} cycling over them (each kind meets each nb)."""
    out = []
    for i, (n, F, nb) in enumerate(SHAPES):
        out.append(random_case(n, F, nb, _KINDS[(i + i // 3) % 3], i % 2,
                               seed=100 + i))
    return out


def _one_bin(cnt, s, nd, f, c, v, b=0):
    """Everything of (nd, f) in one bin: no candidate, either kind."""
    cnt[nd, f, b] = c
    s[nd, f, b] = v


def planted_case(nb=64):
    """n = 8, F = 5 (a partial workgroup of waves), features 1 and 3
    categorical. One hand-stated situation per node; see the comments."""
    n, F = 8, 5
    cnt = torch.zeros(n, F, nb)
    s = torch.zeros(n, F, nb)
    ftype = torch.tensor([0, 8, 0, 8, 0], dtype=torch.int32)
    planted = {}

    # node 0: the winner is continuous: feature 2 steps from -3 to +3 per
    # sample after bin 10; every other feature sits in one bin (for the
    # categorical ones: exactly one live category, no candidate)
    cnt[0, 2, :21] = 4
    s[0, 2, :11] = -12
    s[0, 2, 11:21] = 12
    for f in (0, 1, 3, 4):
        _one_bin(cnt, s, 0, f, 84, -12, b=f)
    planted[0] = (2, 10, 0)

    # node 1: the winner is categorical: feature 3, categories {1, 4, 6} at
    # +5 per sample, the other five at -5; the five share a mean, so the
    # order is 0 2 3 5 7 | 1 4 6
    cnt[1, 3, :8] = 4
    s[1, 3, :8] = -20
    for c in (1, 4, 6):
        s[1, 3, c] = 20
    for f in (0, 1, 2, 4):
        _one_bin(cnt, s, 1, f, 32, -40, b=nb - 1)
    planted[1] = (3, -2, 0x52)

    # node 2: all-zero histograms
    planted[2] = (0, -1, 0)

    # node 3: samples spread over bins, all residual sums zero: every
    # candidate's gain is exactly 0
    cnt[3, :, :6] = 3
    planted[3] = (0, -1, 0)

    # node 4: features 0 and 2 (continuous) and 1 and 3 (categorical) hold
    # the same histogram; the split is clear, and the lowest feature wins
    for f in range(4):
        cnt[4, f, 5] = 6
        s[4, f, 5] = -18
        cnt[4, f, 9] = 6
        s[4, f, 9] = 18
    _one_bin(cnt, s, 4, 4, 12, 0)
    planted[4] = (0, 5, 0)

    # node 5: exactly two live categories, the upper one the last lane
    cnt[5, 1, 7] = 3
    s[5, 1, 7] = -6
    cnt[5, 1, nb - 1] = 5
    s[5, 1, nb - 1] = 10
    for f in (0, 2, 3, 4):
        _one_bin(cnt, s, 5, f, 8, 4, b=1)
    planted[5] = (1, -2, signed64(1 << (nb - 1)))

    # node 6: two categories of equal mean (-1) and one at +3: order 2 5 9,
    # best left = {2, 5}
    for c, k, v in ((2, 2, -2), (5, 4, -4), (9, 3, 9)):
        cnt[6, 3, c] = k
        s[6, 3, c] = v
    for f in (0, 1, 2, 4):
        _one_bin(cnt, s, 6, f, 9, 3, b=2)
    planted[6] = (3, -2, 1 << 9)

    # node 7: all nb categories live: even ids at -1 per sample, odd at +1
    cnt[7, 1, :] = 2
    s[7, 1, 0::2] = -2
    s[7, 1, 1::2] = 2
    for f in (0, 2, 3, 4):
        _one_bin(cnt, s, 7, f, 2 * nb, 0, b=3)
    odd = sum(1 << c for c in range(1, nb, 2))
    planted[7] = (1, -2, signed64(odd))

    return dict(name=f"planted nb{nb}", cnt=cnt, s=s, ftype=ftype, lam=1.0,
                planted=planted)


def all_cases():
    return shape_cases() + [planted_case(64), planted_case(24)]


# ------------------------------------------------------------------- checker

def _gain64(sl, cl, sr, cr, lam):
    """fp64 gain and the sum of the magnitudes of its three terms."""
    stot, ctot = sl + sr, cl + cr
    a, b, c = sl * sl / (cl + lam), sr * sr / (cr + lam), \
        stot * stot / (ctot + lam)
    return a + b - c, a + b + c


def candidates64(cnt, s, categorical, lam):
    """[(gain, terms, threshold, mask)] of one (node, feature) histogram in
    fp64 over the defined candidate set, in candidate order."""
    nb = len(cnt)
    out = []
    if not categorical:
        order = list(range(nb))
    else:
        live = [b for b in range(nb) if cnt[b] > 0]
        order = sorted(live, key=lambda b: (s[b] / cnt[b], b))
    cl = sl = 0.0
    ctot, stot = float(sum(cnt[b] for b in order)), \
        float(sum(s[b] for b in order))
    for p, b in enumerate(order[:-1]):
        cl += cnt[b]
        sl += s[b]
        cr, sr = ctot - cl, stot - sl
        if not (cl > 0 and cr > 0):
            continue
        g, terms = _gain64(sl, cl, sr, cr, lam)
        if categorical:
            out.append((g, terms, -2, sum(1 << c for c in order[p + 1:])))
        else:
            out.append((g, terms, b, 0))
    return out


def check(case, outs, label="", exact_sums=True):
    """Checker items 1-3 of the issue on the op's outputs (any device).
    Returns the worst (best fp64 gain - returned split's fp64 gain) / bound
    over the nodes that split."""
    feature, threshold, mask, gain = [t.cpu() for t in outs]
    cnt = case["cnt"].double().numpy()
    s = case["s"].double().numpy()
    ftype = case["ftype"].tolist()
    lam = case["lam"]
    n, F, nb = cnt.shape
    assert feature.dtype == torch.int32 and threshold.dtype == torch.int32
    assert mask.dtype == torch.int64 and gain.dtype == torch.float32
    assert feature.shape == threshold.shape == mask.shape == gain.shape \
        == (n,)
    worst = 0.0
    for nd in range(n):
        where = f"{label} {case['name']} node {nd}"
        f, t = int(feature[nd]), int(threshold[nd])
        m = unsigned64(int(mask[nd]))
        best, bound = -np.inf, 0.0
        for ff in range(F):
            for g, terms, _, _ in candidates64(cnt[nd, ff], s[nd, ff],
                                               ftype[ff] != 0, lam):
                if g > best:
                    best, bound = g, ULPS * terms
        if nd in case["planted"]:
            assert (f, t, signed64(m)) == case["planted"][nd], where
        if t == -1:
            # pass-through: nothing gains more than the constant, within
            # the rounding bound
            assert f == 0 and m == 0, where
            assert best <= MIN_GAIN + bound, (where, best, bound)
            assert float(gain[nd]) == 0.0, where
            continue
        assert 0 <= f < F, where
        c, v = cnt[nd, f], s[nd, f]
        if t >= 0:
            assert ftype[f] == 0 and t <= nb - 2 and m == 0, where
            right = np.arange(nb) > t
        else:
            assert t == -2 and ftype[f] != 0 and m != 0, where
            assert nb >= 64 or m >> nb == 0, where
            right = np.array([(m >> b) & 1 == 1 if b < 64 else False
                              for b in range(nb)])
            live = c > 0
            assert not (right & ~live).any(), where      # live ones only
            means = v[live] / c[live]
            rmean = means[right[live]]
            lmean = means[~right[live]]
            # the right side is an upper set of the mean order
            assert lmean.size and rmean.size and lmean.max() <= rmean.min(), \
                where
        cl, sl = c[~right].sum(), v[~right].sum()
        cr, sr = c[right].sum(), v[right].sum()
        assert cl > 0 and cr > 0, where
        got, terms = _gain64(sl, cl, sr, cr, lam)
        assert best > MIN_GAIN - bound, (where, best)
        assert got >= best - bound, (where, got, best, bound)
        if exact_sums:
            assert abs(float(gain[nd]) - got) <= ULPS * terms, \
                (where, float(gain[nd]), got)
        if bound > 0:
            worst = max(worst, (best - got) / bound)
    return worst


# ---------------------------------------------------- exhaustive subset search

def exhaustive_best(cnt, s, lam):
    """fp64 optimum of the gain over ALL two-sided partitions of the live
    categories of one histogram (what the reference does by Gray code up to
    10 labels). Returns (gain, terms at the optimum) or None."""
    live = [b for b in range(len(cnt)) if cnt[b] > 0]
    L = len(live)
    if L < 2:
        return None
    c = np.array([cnt[b] for b in live], dtype=np.float64)
    v = np.array([s[b] for b in live], dtype=np.float64)
    # the subsets that hold the first live category, but not all of them
    codes = np.arange(1, 1 << L, 2)[:-1]
    bits = (codes[:, None] >> np.arange(L)) & 1
    cl, sl = bits @ c, bits @ v
    cr, sr = c.sum() - cl, v.sum() - sl
    g, terms = _gain64(sl, cl, sr, cr, lam)
    i = int(np.argmax(g))
    return float(g[i]), float(terms[i])


def returned_gain64(cnt, s, lam, threshold, mask):
    """fp64 gain of a categorical answer on one histogram, None for a
    pass-through."""
    if threshold == -1:
        return None
    m = unsigned64(mask)
    right = np.array([(m >> b) & 1 == 1 for b in range(len(cnt))])
    c, v = np.asarray(cnt, dtype=np.float64), np.asarray(s, dtype=np.float64)
    return float(_gain64(v[~right].sum(), c[~right].sum(), v[right].sum(),
                         c[right].sum(), lam)[0])


def random_categorical(n, nb, max_live, seed):
    """n single-feature categorical histograms with 2..max_live live
    categories: counts 1..20 (every other histogram: 1..3, where lam weighs
    most), sums multiples of 1/8 (exact in fp32)."""
    g = torch.Generator().manual_seed(seed)
    cnt = torch.zeros(n, 1, nb)
    s = torch.zeros(n, 1, nb)
    for i in range(n):
        L = int(torch.randint(2, max_live + 1, (1,), generator=g))
        ids = torch.randperm(nb, generator=g)[:L]
        c = torch.randint(1, 4 if i % 2 else 21, (L,), generator=g).float()
        cnt[i, 0, ids] = c
        s[i, 0, ids] = torch.round(torch.randn(L, generator=g) * c * 8) / 8
    return cnt, s


# ------------------------------------------------------- build_tree fixture

def subset_fixture(device="cpu"):
    """512 rows, F = 3: two continuous noise columns (16 bins) and one
    categorical with 8 categories; y = +1 for categories {1, 4, 6}, else -1.
    Returns (bins int64 [512, 3], y float32 [512], feature_types int32 [3])."""
    g = torch.Generator().manual_seed(7)
    B = 512
    bins = torch.empty(B, 3, dtype=torch.int64)
    bins[:, 0] = torch.randint(0, 16, (B,), generator=g)
    bins[:, 1] = torch.randint(0, 16, (B,), generator=g)
    bins[:, 2] = torch.arange(B) % 8
    bins[:, 2] = bins[torch.randperm(B, generator=g), 2]
    y = torch.where((bins[:, 2] == 1) | (bins[:, 2] == 4)
                    | (bins[:, 2] == 6), 1.0, -1.0)
    types = torch.tensor([0, 0, 8], dtype=torch.int32)
    return bins.to(device), y.to(device), types
