"""GBT — gradient-boosted trees on the PS.

Reference: dolphin/mlapps/gbt/GBTTrainer.java (966 LoC) — model table maps
label -> List<GBTree>; each batch the worker pulls ALL trees (pullAllTrees
:767), computes residuals from the pulled forest, builds ONE tree greedily
(per-node best-split search over features, :244+), and pushes the whole tree
from inside localCompute (pushTree :753; pushUpdate is empty :201-204); the
server appends (GBTETModelUpdateFunction.java:32). Feature types come from a
metadata file (GBTMetadataParser.java).

MI355X redesign: exact per-value split scans are replaced by the standard
GPU-GBT histogram method (K10): features are pre-quantized to NBINS bins
once per data block; each tree level builds (count, sum-residual) histograms
for ALL nodes x features x bins with one scatter-add over the device-resident
batch, and best splits come from a parallel prefix-scan of the histograms —
no per-sample host loops. Trees are flat arrays (feature/bin/leaf tensors)
stored in an object table keyed by label (multi-class = one forest per
label, regression = label 0).

App args: num_features, batch_size, num_bins, max_depth, step_size
(shrinkage), lam (leaf L2), test_data_path, objective ("regression" | "multiclass"
with num_classes — one forest per label in the object table, reference
GBTTrainer's valueTypeNum > 3 path / GroupedTree).

Feature types (feature_types): with `input`, the metadata file (`metadata`,
default <input>.meta) marks a feature continuous (0) or categorical (its
number of categories); synthetic data makes its last `num_categorical`
features categorical with `num_categories` values each. A categorical
column is not binned (bin = category id, so at most min(num_bins, 64)
categories) and is split by a SUBSET of its categories (K10b, reference
bestSplitLabelFeature), stored per node as a 64-bit mask. Without a
categorical feature nothing changes.

sparse=true (default false; nnz_per_row for synthetic data) keeps every
block as a SparseBins (mlapps/sparse_bins.py; reference GBTETDataParser
createSparse): CSR input is binned without densifying, with the edges
quantize gives the densified block, the level histograms come from K10s
(ops.gbt_hist_sparse) over the features present in the block, and routing
and prediction look a bin up instead of gathering it from a dense row. On
the same data the trees equal the dense path's; memory and time follow nnz
and the number of present features, never B * F.

test_data_path (mlapps/heldout.py; reference TestDataProvider): a held-out
file, read whole by every rank in build() and kept as ONE block, binned
exactly as a training block is (quantize / SparseBins with the job's feature
types, the same ValueError for a bad category). evaluate_test() applies the
whole forest to it with gbt.forest_predict (K10p, ops.gbt_forest_predict) and
reports test_mse (regression) or test_error_rate (multiclass) with
test_examples. Binning semantics: a tree here stores BIN INDICES, and every
block is binned by its own quantiles, so the forest is applied to the test
set's own quantile bins, the same way it is applied to every training block.
Job-wide bin edges stored with the model would change training results and
are not built (docs/ROADMAP.md).
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import torch

from harmony_amd.config import JobConfig, TableConfig
from harmony_amd.dolphin.data_provider import TrainingDataProvider
from harmony_amd.dolphin.trainer import Trainer, TrainerContext
from harmony_amd.et.table import ObjectTable
from harmony_amd.mlapps import heldout
from harmony_amd.mlapps.sparse_batch import (csr_row_blocks, drop_repeats,
                                             is_sparse, reslice)
from harmony_amd.mlapps.sparse_bins import SparseBins
from harmony_amd.utils import stable_seed
from harmony_amd import ops

MODEL_TABLE = "gbt_model"


def defaults(job: JobConfig) -> dict:
    a = dict(num_features=32, batch_size=4096, num_bins=64, max_depth=4,
             step_size=0.1, lam=1.0, noise=0.1, objective="regression",
             num_classes=3, num_categorical=0, num_categories=8,
             sparse="false", nnz_per_row=32)
    a.update(job.app_args)
    return a


@dataclass
class GBTree:
    """Flat complete binary tree of depth d: internal nodes 0..2^d-2 hold
    (feature, bin_threshold); leaves hold values. Node kinds by threshold t:
    t >= 0 continuous, right iff bin > t; t == -1 pass-through, always left;
    t == -2 categorical, right iff bit `bin` of cat_mask[node] is set (a
    category outside the mask, seen while building or not, goes left).
    cat_mask is None for a tree built without feature types; the class-level
    default also serves trees pickled before the field existed."""

    depth: int
    feature: List[int]          # [2^d - 1]
    threshold: List[int]        # [2^d - 1] (bin index; -1, -2: see above)
    leaf_value: List[float]     # [2^d]
    cat_mask: Optional[List[int]] = None   # [2^d - 1] signed 64-bit masks

    def predict_bins(self, bins) -> torch.Tensor:
        """bins: [B, F] int64 quantized features, or a SparseBins of that
        shape (a bin is then looked up, not gathered) -> [B] predictions."""
        # without masks no node is categorical (t == -2)
        masks = self.cat_mask if self.cat_mask is not None \
            else [0] * len(self.feature)
        rows = torch.tensor([self.feature, self.threshold, masks],
                            dtype=torch.int64, device=bins.device)
        # the level-local node per sample, as in _grow
        local = torch.zeros(bins.shape[0], dtype=torch.int64,
                            device=bins.device)
        for level in range(self.depth):
            first = 2 ** level - 1
            feat, thr, mask = rows[:, first:2 * first + 1][:, local]
            go_right = _route_right(_bin_of(bins, feat), thr, mask)
            local = torch.add(go_right, local, alpha=2)
        lv = torch.tensor(self.leaf_value, device=bins.device)
        return lv[local]


def _bin_of(bins, feat: torch.Tensor) -> torch.Tensor:
    """int64 [B]: the bin of feature feat[i] in row i of dense bins or of a
    SparseBins (a lookup instead of a gather)."""
    if isinstance(bins, SparseBins):
        return bins.bin_of(feat)
    return bins.gather(1, feat.unsqueeze(1)).squeeze(1)


def _route_right(b: torch.Tensor, t: torch.Tensor, m: torch.Tensor
                 ) -> torch.Tensor:
    """go-right per sample from its bin b, and its node's threshold t and
    category mask m (int64): the three node kinds of GBTree."""
    in_mask = ((m >> b.clamp(0, 63)) & 1).bool() & (b < 64)
    return torch.where(t >= 0, b > t, (t == -2) & in_mask)


def encode_trees(items, depth: int) -> torch.Tensor:
    """Tensor codec for a FIXED-count batch of (key, GBTree) items: one
    int32 row per tree = [key, feature[2^d-1], threshold[2^d-1],
    bitcast(leaf f32)[2^d]]. Replaces the pickled wire (GBTreeListCodec in
    the reference, mlapps/serialization/) with a flat all-gatherable
    tensor — VERDICT r01 weak #4.

    If any tree of the batch has a cat_mask, every row is extended by
    2 * (2^d - 1) words, the low and the high half of each node's mask as
    bit patterns (a tree without masks sends zeros), so the rows of a batch
    are always equally long."""
    ni = (1 << depth) - 1
    with_masks = any(t.cat_mask is not None for _, t in items)
    rows = []
    for key, t in items:
        assert t.depth == depth
        parts = [
            torch.tensor([key], dtype=torch.int32),
            torch.tensor(t.feature, dtype=torch.int32),
            torch.tensor(t.threshold, dtype=torch.int32),
            torch.tensor(t.leaf_value,
                         dtype=torch.float32).view(torch.int32)]
        if with_masks:
            m = torch.tensor(t.cat_mask if t.cat_mask is not None
                             else [0] * ni, dtype=torch.int64)
            halves = m.view(torch.int32).view(ni, 2)    # little-endian
            parts += [halves[:, 0].contiguous(), halves[:, 1].contiguous()]
        rows.append(torch.cat(parts))
    return torch.stack(rows) if rows else torch.empty((0, 1 + 2 * ni +
                                                       (1 << depth)),
                                                      dtype=torch.int32)


def decode_trees(enc, depth: int):
    """enc: the [n, row] tensor of encode_trees, or a sequence of 1-D rows.
    A row of 1 + 2 ni + 2^d words is a tree without masks; 2 ni words more
    carry the masks."""
    ni = (1 << depth) - 1
    base = 1 + 2 * ni + (1 << depth)
    out = []
    rows = enc.cpu() if isinstance(enc, torch.Tensor) else enc
    for row in rows:
        row = row.cpu()
        assert row.shape[0] in (base, base + 2 * ni), row.shape
        key = int(row[0])
        feat = row[1:1 + ni].tolist()
        thr = row[1 + ni:1 + 2 * ni].tolist()
        lv = row[1 + 2 * ni:base].view(torch.float32).tolist()
        masks = None
        if row.shape[0] > base:
            halves = torch.stack([row[base:base + ni],
                                  row[base + ni:base + 2 * ni]], dim=1)
            masks = halves.contiguous().view(torch.int64).view(ni).tolist()
        out.append((key, GBTree(depth=depth, feature=feat, threshold=thr,
                                leaf_value=lv, cat_mask=masks)))
    return out


def pack_forest(forest: List[GBTree], depth: int) -> torch.Tensor:
    """The device format of a forest: the int32 [T, row] tensor
    encode_trees gives for [(0, tree), ...] (key word 0), one row per tree in
    forest order. Built column block by column block, one host tensor per
    block instead of encode_trees' four to six per tree (about a tenth of
    its time at 1024 trees; tests/test_gbt_predict_cpu.py holds the two
    equal)."""
    if not forest:
        return encode_trees([], depth)
    ni = (1 << depth) - 1
    assert all(t.depth == depth for t in forest)
    parts = [
        torch.tensor([[0] + t.feature + t.threshold for t in forest],
                     dtype=torch.int32),
        torch.tensor([t.leaf_value for t in forest],
                     dtype=torch.float32).view(torch.int32)]
    if any(t.cat_mask is not None for t in forest):
        m = torch.tensor([t.cat_mask if t.cat_mask is not None else [0] * ni
                          for t in forest], dtype=torch.int64)
        halves = m.view(torch.int32).view(len(forest), ni, 2)  # little-endian
        parts += [halves[:, :, 0], halves[:, :, 1]]
    return torch.cat(parts, dim=1).contiguous()


# Trees from which forest_predict packs the forest and runs K10p; below it
# the per-tree predict_bins loop stays. Measured (profiles/gbt_predict_ab.md):
# K10p with its pack time wins from a single tree on, dense and sparse.
FOREST_KERNEL_MIN_TREES = 1


def forest_predict(forest: List[GBTree], bins, step_size: float
                   ) -> torch.Tensor:
    """step_size * the forest's prediction for dense bins or a SparseBins,
    float32 [B]: what GBTTrainer._forest_pred gives from an empty cache, bit
    for bit, in one launch on the device (ops.gbt_forest_predict)."""
    if len(forest) < max(1, FOREST_KERNEL_MIN_TREES):
        pred = torch.zeros(bins.shape[0], dtype=torch.float32,
                           device=bins.device)
        for t in forest:
            pred = pred + step_size * t.predict_bins(bins)
        return pred
    depth = forest[0].depth
    return ops.gbt_forest_predict(bins, pack_forest(forest, depth), depth,
                                  step_size)


MAX_CATEGORIES = 64    # a node's categories are one 64-bit mask
CAT_EFFECT = 3.0       # synthetic data: size of the category-subset term


def feature_types(app_args: dict) -> Optional[torch.Tensor]:
    """The job's feature types: int32 [num_features], 0 = continuous,
    non-zero = categorical (the number of categories), or None when no
    feature is categorical. With `input` they come from the metadata file
    (`metadata`, default <input>.meta; reference GBTMetadataParser): entries
    at or past num_features (the y-value entry) are ignored, a feature the
    file does not name is continuous, a missing file means no types.
    Synthetic data: the last num_categorical features."""
    F = int(app_args.get("num_features", 32))
    types = torch.zeros(F, dtype=torch.int32)
    if app_args.get("input"):
        from harmony_amd import dataloader as dl

        meta_path = app_args.get("metadata", app_args["input"] + ".meta")
        try:
            meta = dl.parse_gbt_meta(dl.read_split(meta_path, (0, 1 << 50)))
        except OSError:
            meta = {}
        for i, t in meta.items():
            if 0 <= i < F:
                types[i] = t
    else:
        nc = int(app_args.get("num_categorical", 0))
        if nc > 0:
            types[max(0, F - nc):] = int(app_args.get("num_categories", 8))
    return types if bool((types != 0).any()) else None


def quantize(X: torch.Tensor, num_bins: int,
             feature_types: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-feature quantile binning (reference pre-sorts per feature for the
    exact scan; binning is the histogram-method equivalent). A column that
    feature_types marks categorical is not binned: bin = int(value), which
    must be an integer in 0 .. min(num_bins, 64) - 1."""
    qs = torch.quantile(X, torch.linspace(0, 1, num_bins + 1,
                                          device=X.device)[1:-1], dim=0)
    bins = torch.searchsorted(qs.t().contiguous(), X.t().contiguous()
                              ).t().contiguous().clamp_(0, num_bins - 1)
    if feature_types is None:
        return bins
    limit = min(num_bins, MAX_CATEGORIES)
    for f in (feature_types != 0).nonzero().flatten().tolist():
        col = X[:, f]
        bad = (col < 0) | (col != col.floor()) | (col >= limit) \
            | ~torch.isfinite(col)
        if bool(bad.any()):
            v = float(col[bad][0])
            raise ValueError(
                f"categorical feature {f}: value {v!r} is not an integer in "
                f"0..{limit - 1} (cardinality is limited by num_bins = "
                f"{num_bins} and {MAX_CATEGORIES})")
        bins[:, f] = col.long()
    return bins


def build_tree(bins: torch.Tensor, resid: torch.Tensor, num_bins: int,
               max_depth: int, lam: float,
               feature_types: Optional[torch.Tensor] = None) -> GBTree:
    """Level-wise histogram tree build (_grow): per level one histogram of
    (count, sum) for all nodes and one split search; split gain = variance
    reduction. The kinds of input differ in these two steps only:

    dense bins, no feature_types: K10 (ops.gbt_hist) and the tensor-op
    threshold search (_threshold_search);
    dense bins with feature_types (even all zeros): K10 and
    ops.gbt_best_split (K10b), which also searches category subsets;
    SparseBins: K10s and K10b over the batch's present features, the winner
    mapped back through feat_ids. A feature absent from the batch has one
    populated bin and so no valid candidate: leaving it out changes no
    winner, and feat_ids ascending keeps the lowest-feature tie rule, so the
    trees are the ones the dense bins of the same data give. Without
    feature types the types are zeros.

    The tree has cat_mask = None exactly when feature_types is None."""
    dev = bins.device
    if isinstance(bins, SparseBins):
        ids = bins.feat_ids.long()
        nf = ids.shape[0]
        if feature_types is None:
            ftype = torch.zeros(nf, dtype=torch.int32, device=dev)
        else:
            ftype = feature_types.to(device=dev, dtype=torch.int32)[ids]

        def split(local, n_nodes):
            if nf == 0:
                feat = torch.zeros(n_nodes, dtype=torch.int64, device=dev)
                return feat, feat - 1, feat.clone()
            cnt, s = ops.gbt_hist_sparse(
                bins.feat_ptr, bins.feat_row, bins.feat_bin, bins.feat_idx,
                bins.zero_bin, resid, local, n_nodes, num_bins)
            feat, thr, mask, _ = ops.gbt_best_split(cnt, s, ftype, lam)
            thr = thr.long()
            # a no-split node reports feature 0, as K10b does on dense bins
            return torch.where(thr == -1, torch.zeros_like(thr),
                               ids[feat.long()]), thr, mask
    elif feature_types is None:
        def split(local, n_nodes):
            cnt, s = ops.gbt_hist(bins, resid, local, n_nodes, num_bins)
            return _threshold_search(cnt, s, lam)
    else:
        ftype = feature_types.to(device=dev, dtype=torch.int32)

        def split(local, n_nodes):
            cnt, s = ops.gbt_hist(bins, resid, local, n_nodes, num_bins)
            feat, thr, mask, _ = ops.gbt_best_split(cnt, s, ftype, lam)
            return feat.long(), thr.long(), mask
    return _grow(bins, resid, max_depth, lam, split,
                 with_masks=feature_types is not None)


def _threshold_search(cnt: torch.Tensor, s: torch.Tensor, lam: float):
    """Best threshold split per node from [n_nodes, F, nb] histograms, with
    tensor ops: (feature, threshold, mask) int64 [n_nodes]. The feature of
    the best candidate is reported even for a node that does not split
    (threshold -1); the masks are zero."""
    n_nodes, _, num_bins = cnt.shape
    # prefix sums over bins: left side of split at bin b = bins <= b
    ccum = cnt.cumsum(dim=2)
    scum = s.cumsum(dim=2)
    ctot = ccum[:, :, -1:]
    stot = scum[:, :, -1:]
    cl, sl = ccum[:, :, :-1], scum[:, :, :-1]
    cr, sr = ctot - cl, stot - sl
    # gain = sl^2/(cl+lam) + sr^2/(cr+lam) - stot^2/(ctot+lam)
    gain = (sl * sl / (cl + lam) + sr * sr / (cr + lam)
            - stot * stot / (ctot + lam))
    gain = torch.where((cl > 0) & (cr > 0), gain,
                       torch.full_like(gain, -1e30))
    flat = gain.view(n_nodes, -1)
    best = flat.argmax(dim=1)
    best_gain = flat.gather(1, best.unsqueeze(1)).squeeze(1)
    thr = torch.where(best_gain > 1e-12, best % (num_bins - 1), -1)
    return best // (num_bins - 1), thr, torch.zeros_like(best)


def _leaf_values(leaf: torch.Tensor, resid: torch.Tensor, n_leaves: int,
                 lam: float) -> List[float]:
    """sum(resid) / (count + lam) per leaf, from the samples' leaves."""
    cnt = torch.zeros(n_leaves, device=leaf.device).scatter_add_(
        0, leaf, torch.ones_like(resid))
    s = torch.zeros(n_leaves, device=leaf.device).scatter_add_(0, leaf, resid)
    return (s / (cnt + lam)).tolist()


def _grow(bins, resid: torch.Tensor, max_depth: int, lam: float, split,
          with_masks: bool) -> GBTree:
    """The level loop of build_tree. split(local, n_nodes) -> (feature,
    threshold, mask), int64 [n_nodes] each in global feature numbers, is the
    level's histogram and split search for samples at level-local nodes
    `local` (node 2^level - 1 + local of the tree). Per level there is ONE
    host copy, of the stacked (feature, threshold, mask) rows for the tree's
    lists; the routing runs on the device from the same tensor."""
    local = torch.zeros(bins.shape[0], dtype=torch.int64, device=bins.device)
    feature: List[int] = []
    threshold: List[int] = []
    cat_mask: List[int] = []
    for level in range(max_depth):
        rows = torch.stack(split(local, 2 ** level))        # [3, n_nodes]
        f_l, t_l, m_l = rows.tolist()
        feature += f_l
        threshold += t_l
        cat_mask += m_l
        feat, thr, mask = rows[:, local]
        go_right = _route_right(_bin_of(bins, feat), thr, mask)
        # the children of local node i are 2 i and 2 i + 1 of the next level
        local = torch.add(go_right, local, alpha=2)
    return GBTree(max_depth, feature, threshold,
                  _leaf_values(local, resid, 2 ** max_depth, lam),
                  cat_mask if with_masks else None)


class GBTTrainer(Trainer):
    def __init__(self, ctx: TrainerContext):
        super().__init__(ctx)
        self.a = defaults(JobConfig(job_id=ctx.job_id, app="gbt",
                                    app_args=ctx.app_args))
        self.table: ObjectTable = ctx.table(MODEL_TABLE)
        self.forest: List[GBTree] = []
        self.forests: List[List[GBTree]] = []
        self._mc_cache: dict = {}
        self._mse = 0.0
        # incremental forest predictions: the forest is append-only
        # (update fn v + [d]), so each block's prediction is cached and only
        # trees added since the block's last visit are applied — O(new)
        # instead of O(total) trees per batch
        self._pred_cache: dict = {}
        # resolved once; every build_tree call gets them (None: no
        # categorical feature, the untyped split search)
        ft = feature_types(self.a)
        self.feature_types = None if ft is None else ft.to(ctx.device)

    def pull_model(self) -> None:
        # pullAllTrees (reference :767). The forest is APPEND-ONLY, so
        # every rank keeps a full replica updated incrementally by the
        # tensorized push sync (push_update) — steady-state pulls move
        # ZERO bytes. The pickled gather remains only as the rebuild path
        # after out-of-band content changes (restore/migration/puts).
        ce = getattr(self.table, "content_epoch", 0)
        ov = self.table.ownership.version
        if getattr(self, "_replica", None) is None or \
                self._replica_stamp != (ce, ov):
            allv = self.table.pull_all()
            self._replica = {k: list(v) for k, v in allv.items()}
            self._replica_stamp = (ce, ov)
        allv = self._replica
        if self.a["objective"] == "multiclass":
            C = self.a["num_classes"]
            self.forests = [allv.setdefault(c, []) for c in range(C)]
        else:
            self.forest = allv.setdefault(0, [])

    def _trivial_tree(self):
        # a stopped worker still contributes to the equal-count tree
        # all-gather: a pass-through tree predicting 0 (harmless append)
        d = self.a["max_depth"]
        # with typed features every rank encodes the extended tree row
        typed = getattr(self, "feature_types", None) is not None
        return GBTree(depth=d, feature=[0] * ((1 << d) - 1),
                      threshold=[-1] * ((1 << d) - 1),
                      leaf_value=[0.0] * (1 << d),
                      cat_mask=[0] * ((1 << d) - 1) if typed else None)

    @staticmethod
    def _forest_pred(cache: dict, key, forest: List[GBTree], bins,
                     like: torch.Tensor, step_size: float) -> torch.Tensor:
        """step_size * the forest's prediction for bins, from the cache
        entry (done, last, pred) under `key`: only trees past `done` are
        applied, and the entry is renewed."""
        done, last, pred = cache.get(key, (0, None, None))
        # valid only if the cached prefix is literally this forest's prefix
        # (offline eval may reload an older/replaced forest into the table)
        if pred is None or done > len(forest) or (
                done > 0 and forest[done - 1] is not last):
            done, pred = 0, torch.zeros_like(like)
        for t in forest[done:]:
            pred = pred + step_size * t.predict_bins(bins)
        cache[key] = (len(forest), forest[-1] if forest else None, pred)
        return pred

    def local_compute(self) -> None:
        if self.batch[0].shape[0] == 0:
            if self.a["objective"] == "multiclass":
                self.new_trees = [(c, self._trivial_tree())
                                  for c in range(self.a["num_classes"])]
            else:
                self.new_tree = self._trivial_tree()
            self._mse = 0.0
            return
        if self.a["objective"] == "multiclass":
            self._compute_multiclass()
            return
        bins, y = self.batch
        a = self.a
        pred = GBTTrainer._forest_pred(self._pred_cache, id(self.batch),
                                       self.forest, bins, y, a["step_size"])
        resid = y - pred
        self._mse = float((resid * resid).mean())
        self.new_tree = build_tree(bins, resid, a["num_bins"], a["max_depth"],
                                   a["lam"],
                                   getattr(self, "feature_types", None))

    def _compute_multiclass(self) -> None:
        """One-vs-all boosting (reference GBTTrainer multi-label: one GBTree
        forest per label type): per class, residual = onehot - sigmoid-free
        additive score, one new tree per class per batch."""
        bins, y = self.batch
        a = self.a
        C = a["num_classes"]
        self.new_trees = []
        scores = []
        for c in range(C):
            target = (y == c).float()
            pred = GBTTrainer._forest_pred(
                self._mc_cache, (id(self.batch), c), self.forests[c], bins,
                target, a["step_size"])
            resid = target - pred
            scores.append(pred)
            self.new_trees.append(
                (c, build_tree(bins, resid, a["num_bins"], a["max_depth"],
                               a["lam"],
                               getattr(self, "feature_types", None))))
        pred_cls = torch.stack(scores, dim=1).argmax(dim=1)
        self._mse = float((pred_cls != y.long()).float().mean())  # error rate

    def push_update(self) -> None:
        # reference pushes the tree from localCompute; here the push phase
        # does it so NET ordering holds. Wire = ONE all-gather of a flat
        # int32 tensor (every rank pushes exactly one tree per class per
        # batch, so counts are equal by construction); each rank decodes
        # all contributions, appends them to its replica in rank order,
        # and owners append to the object table (authoritative store for
        # checkpoint/migration).
        items = (self.new_trees if self.a["objective"] == "multiclass"
                 else [(0, self.new_tree)])
        comm = self.table.comm
        if comm is None or self.table.world_size == 1:
            for key, tree in items:
                self.table.update_local(key, tree)
                if getattr(self, "_replica", None) is not None:
                    self._replica.setdefault(key, []).append(tree)
            return
        enc = encode_trees(items, self.a["max_depth"])
        per_rank = comm.gather_equal(enc)
        my_blocks = set(self.table.blocks.keys())
        for renc in per_rank:
            for key, tree in decode_trees(renc, self.a["max_depth"]):
                if self._replica is not None:
                    self._replica.setdefault(key, []).append(tree)
                if self.table.part.block_of_int(key) in my_blocks:
                    self.table.update_local(key, tree)

    def evaluate_model(self):
        if self.a["objective"] == "multiclass":
            n = float(sum(len(f) for f in self.forests))
            return {"error_rate": self._mse, "num_trees": n}
        return {"mse": self._mse, "num_trees": float(len(self.forest))}

    def evaluate_test(self):
        """The current forest on the held-out block: one forest_predict per
        forest. Training state (_mse, the prediction caches) is not
        touched; pull_model only refreshes the replica, as the next batch
        would."""
        if not self.test_blocks:
            return {}
        self.pull_model()
        bins, y = self.test_blocks[0]
        step = self.a["step_size"]
        out = {"test_examples": float(y.shape[0])}
        if self.a["objective"] == "multiclass":
            scores = [forest_predict(f, bins, step) for f in self.forests]
            pred_cls = torch.stack(scores, dim=1).argmax(dim=1)
            out["test_error_rate"] = float(
                (pred_cls != y.long()).float().mean())
        else:
            resid = y - forest_predict(self.forest, bins, step)
            out["test_mse"] = float((resid * resid).mean())
        return out

    def num_batch_examples(self) -> int:
        return self.batch[0].shape[0]


_is_sparse = is_sparse


SPARSE_SIGNAL_COLS = 4   # synthetic sparse data: columns y depends on


def _make_sparse_batches(job: JobConfig, a: dict, rank: int,
                         device: torch.device, world_size: int, ftypes):
    """make_batches for sparse=true: the same block structure as the dense
    branch, every block a (SparseBins, y) pair, binned on the CPU from its
    CSR rows. No tensor with B*F elements is built."""
    F = int(a["num_features"])
    nb = int(a["num_bins"])
    n_blocks = max(1, job.num_worker_blocks or job.num_mini_batches)
    blocks = []
    if a.get("input"):
        from harmony_amd import dataloader as dl

        row_ptr, col, val, y = dl.parse_libsvm_csr_split(
            a["input"], rank, world_size, F)
        for lo, hi, *csr in csr_row_blocks(row_ptr, col, val, y.shape[0],
                                           n_blocks):
            blocks.append((SparseBins((*csr, F), nb, ftypes).to(device),
                           y[lo:hi].float().to(device)))
        return blocks
    B = int(a["batch_size"])
    nc = min(int(a["num_categorical"]), F)
    ncat = int(a["num_categories"])
    k = max(1, min(int(a["nnz_per_row"]), F))
    # y depends on the first ns columns, each present in about half of the
    # rows (an absent one counts as 0.0), so trees find something; with
    # categorical columns the first of them is present in every row
    ns = max(0, min(SPARSE_SIGNAL_COLS, k, F - nc))
    cat_slot = nc > 0 and k > ns
    mc = a["objective"] == "multiclass"
    g = torch.Generator().manual_seed(stable_seed(job.job_id, "data", rank))
    w = torch.randn(max(ns, 1), generator=g) * 2
    if mc:
        W = torch.randn(a["num_classes"], max(ns, 1), generator=g) * 2
    for _ in range(n_blocks):
        # per-row random feature subset: k draws, sorted, repeats dropped
        cols = torch.randint(0, F, (B, k), generator=g)
        if ns > 0:
            sig = torch.rand(B, ns, generator=g) < 0.5
            cols[:, :ns] = torch.where(sig, torch.arange(ns).expand(B, ns),
                                       cols[:, :ns])
        if cat_slot:
            cols[:, ns] = F - nc
        cols = cols.sort(dim=1).values
        keep, row_ptr = drop_repeats(cols)
        vals = torch.randn(B, k, generator=g)
        if nc > 0:
            cats = torch.randint(0, ncat, (B, k), generator=g)
            vals = torch.where(cols >= F - nc, cats.float(), vals)
        # the signal columns' values per row, 0.0 where absent
        xs = torch.stack([(vals * ((cols == j) & keep)).sum(dim=1)
                          for j in range(ns)], dim=1) if ns > 0 \
            else torch.zeros(B, 1)
        effect = torch.zeros(B)
        if cat_slot:
            c0 = (vals * ((cols == F - nc) & keep)).sum(dim=1).long()
            effect = CAT_EFFECT * ((c0 % 3 == 1).float() * 2 - 1)
        if mc:
            score = xs @ W.t()
            score[:, 0] += effect
            y = (score + a["noise"]
                 * torch.randn(B, a["num_classes"], generator=g)
                 ).argmax(dim=1).float()
        else:
            y = xs @ w + torch.sin(3 * xs[:, 0]) * 2 + effect \
                + a["noise"] * torch.randn(B, generator=g)
        x = SparseBins((row_ptr, cols[keep], vals[keep], F), nb, ftypes)
        blocks.append((x.to(device), y.to(device)))
    return blocks


def make_batches(job: JobConfig, rank: int, device: torch.device,
                 world_size: int = 1):
    a = defaults(job)
    F = a["num_features"]
    n_blocks = job.num_worker_blocks or job.num_mini_batches
    ftypes = feature_types(a)
    if _is_sparse(a):
        return _make_sparse_batches(job, a, rank, device, world_size, ftypes)
    if job.app_args.get("input"):
        # sample_gbt libsvm-style rows (+ optional .meta feature types,
        # reference GBTMetadataParser: a categorical column stays unbinned)
        from harmony_amd import dataloader as dl

        X, y = dl.parse_libsvm_split(job.app_args["input"], rank,
                                     world_size, F)
        blocks = []
        for xb, yb in zip(torch.chunk(X, n_blocks), torch.chunk(y, n_blocks)):
            bins = quantize(xb, a["num_bins"], ftypes)
            blocks.append((bins.to(device), yb.to(device)))
        return blocks
    nc = min(int(a["num_categorical"]), F)
    ncat = int(a["num_categories"])
    g = torch.Generator().manual_seed(stable_seed(job.job_id, "data", rank))
    w = torch.randn(F, generator=g)
    mc = a["objective"] == "multiclass"
    if mc:
        W = torch.randn(a["num_classes"], F, generator=g)
    blocks = []
    n_blocks = job.num_worker_blocks or job.num_mini_batches
    for _ in range(n_blocks):
        X = torch.randn(a["batch_size"], F, generator=g)
        if nc > 0:
            # the last nc features are category ids; they stay out of the
            # linear term, and the first of them acts through a fixed
            # non-contiguous subset of its categories (ids = 1 mod 3), which
            # no single ordinal threshold isolates
            cats = torch.randint(0, ncat, (a["batch_size"], nc), generator=g)
            Xc = X.clone()
            Xc[:, F - nc:] = cats.float()
            X[:, F - nc:] = 0.0
            effect = CAT_EFFECT * ((cats[:, 0] % 3 == 1).float() * 2 - 1)
        if mc:
            # separable class labels: argmax of per-class linear scores
            score = X @ W.t()
            if nc > 0:
                score[:, 0] += effect
            y = (score + a["noise"]
                 * torch.randn(a["batch_size"], a["num_classes"],
                               generator=g)).argmax(dim=1).float()
        else:
            y = X @ w + torch.sin(3 * X[:, 0]) * 2
            if nc > 0:
                y = y + effect
            y = y + a["noise"] * torch.randn(a["batch_size"], generator=g)
        if nc > 0:
            X = Xc
        bins = quantize(X, a["num_bins"], ftypes)
        blocks.append((bins.to(device), y.to(device)))
    return blocks


def make_test_block(job: JobConfig, device: torch.device):
    """The held-out file of test_data_path as ONE (bins, y) block, binned as
    a training block is; [] without the arg. Every rank reads the whole
    file."""
    a = defaults(job)
    path = heldout.test_path(a)
    if path is None:
        return []
    F, nb = int(a["num_features"]), int(a["num_bins"])
    ftypes = feature_types(a)
    if _is_sparse(a):
        row_ptr, col, val, y = heldout.load_rows(path, F, True)
        x = SparseBins((row_ptr, col, val, F), nb, ftypes)
    else:
        X, y = heldout.load_rows(path, F, False)
        x = quantize(X, nb, ftypes)
    return [(x.to(device), y.float().to(device))]


def build(job: JobConfig, ctx, cp):
    # before anything else: a missing test file fails the job at once
    test_blocks = make_test_block(job, ctx.device)
    cfg = TableConfig(table_id=f"{job.job_id}/{MODEL_TABLE}", num_keys=16,
                      num_blocks=16, storage="object")
    comm = ctx.new_data_plane()
    table = ObjectTable(cfg, ctx.rank, ctx.world_size, comm=comm,
                        init_value=lambda k: [],
                        update_value=lambda v, d: v + [d])
    tctx = TrainerContext(job_id=job.job_id, rank=ctx.rank,
                          world_size=ctx.world_size, device=ctx.device,
                          tables={MODEL_TABLE: table}, app_args=job.app_args)
    trainer = GBTTrainer(tctx)
    trainer.test_blocks = test_blocks
    provider = TrainingDataProvider(reslice=reslice, local_blocks=
        make_batches(job, ctx.rank, ctx.device, ctx.world_size))
    return {MODEL_TABLE: table}, trainer, provider
