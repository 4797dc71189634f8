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
(shrinkage), lam (leaf L2), objective ("regression" | "multiclass"
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
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import torch

from harmony_amd.config import JobConfig, TableConfig
from harmony_amd.dolphin.data_provider import TrainingDataProvider
from harmony_amd.dolphin.trainer import Trainer, TrainerContext
from harmony_amd.et.table import ObjectTable
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
        sparse = isinstance(bins, SparseBins)
        B = bins.shape[0]
        node = torch.zeros(B, dtype=torch.int64, device=bins.device)
        feat = torch.tensor(self.feature, device=bins.device)
        thr = torch.tensor(self.threshold, device=bins.device)
        cm = None
        if self.cat_mask is not None:
            cm = torch.tensor(self.cat_mask, dtype=torch.int64,
                              device=bins.device)
        for _ in range(self.depth):
            f = feat[node]
            t = thr[node]
            b = bins.bin_of(f) if sparse else \
                bins.gather(1, f.unsqueeze(1)).squeeze(1)
            if cm is None:
                go_right = (b > t) & (t >= 0)
            else:
                go_right = _route_right(b, t, cm[node])
            node = node * 2 + 1 + go_right.long()
        leaf = node - (2 ** self.depth - 1)
        lv = torch.tensor(self.leaf_value, device=bins.device)
        return lv[leaf]


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
    """Level-wise histogram tree build (K10): one scatter-add per level for
    all nodes' (count, sum) histograms; split gain = variance reduction.
    With feature_types (even all zeros) the split search is ops.gbt_best_split
    (K10b), which also searches category subsets; without, the tensor-op
    threshold search below. A SparseBins batch is built by K10s and K10b
    over its present features (_build_tree_sparse) and gives the trees the
    dense bins of the same data give."""
    if isinstance(bins, SparseBins):
        return _build_tree_sparse(bins, resid, num_bins, max_depth, lam,
                                  feature_types)
    if feature_types is not None:
        return _build_tree_typed(bins, resid, num_bins, max_depth, lam,
                                 feature_types)
    B, F = bins.shape
    dev = bins.device
    node = torch.zeros(B, dtype=torch.int64, device=dev)   # node per sample
    n_internal = 2 ** max_depth - 1
    feature = [0] * n_internal
    threshold = [-1] * n_internal
    for level in range(max_depth):
        first = 2 ** level - 1
        n_nodes = 2 ** level
        # histogram: [n_nodes, F, num_bins] counts and residual sums
        # (K10 LDS-privatized kernel on GPU, scatter_add reference on CPU)
        cnt, s = ops.gbt_hist(bins, resid, node - first, n_nodes, num_bins)
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
        bf = (best // (num_bins - 1)).tolist()
        bb = (best % (num_bins - 1)).tolist()
        has_split = (best_gain > 1e-12).tolist()
        for i in range(n_nodes):
            feature[first + i] = int(bf[i])
            threshold[first + i] = int(bb[i]) if has_split[i] else -1
        # route samples
        f_of_node = torch.tensor(feature, device=dev)[node]
        t_of_node = torch.tensor(threshold, device=dev)[node]
        go_right = (bins.gather(1, f_of_node.unsqueeze(1)).squeeze(1)
                    > t_of_node) & (t_of_node >= 0)
        node = node * 2 + 1 + go_right.long()
    # leaves
    first_leaf = 2 ** max_depth - 1
    n_leaves = 2 ** max_depth
    leaf = node - first_leaf
    cnt = torch.zeros(n_leaves, device=dev).scatter_add_(
        0, leaf, torch.ones_like(resid))
    s = torch.zeros(n_leaves, device=dev).scatter_add_(0, leaf, resid)
    values = (s / (cnt + lam)).tolist()
    return GBTree(max_depth, feature, threshold, values)


def _build_tree_typed(bins: torch.Tensor, resid: torch.Tensor, num_bins: int,
                      max_depth: int, lam: float,
                      feature_types: torch.Tensor) -> GBTree:
    """build_tree over typed features: per level K10, K10b, ONE host copy of
    the level's (feature, threshold, mask) rows for the tree's lists, and
    the routing on the device from the same tensors."""
    B, F = bins.shape
    dev = bins.device
    ftype = feature_types.to(device=dev, dtype=torch.int32)
    node = torch.zeros(B, dtype=torch.int64, device=dev)
    feature: List[int] = []
    threshold: List[int] = []
    cat_mask: List[int] = []
    for level in range(max_depth):
        first = 2 ** level - 1
        n_nodes = 2 ** level
        local = node - first
        cnt, s = ops.gbt_hist(bins, resid, local, n_nodes, num_bins)
        feat, thr, mask, _ = ops.gbt_best_split(cnt, s, ftype, lam)
        feat, thr = feat.long(), thr.long()
        f_l, t_l, m_l = torch.stack([feat, thr, mask]).tolist()
        feature += f_l
        threshold += t_l
        cat_mask += m_l
        b = bins.gather(1, feat[local].unsqueeze(1)).squeeze(1)
        go_right = _route_right(b, thr[local], mask[local])
        node = node * 2 + 1 + go_right.long()
    first_leaf = 2 ** max_depth - 1
    n_leaves = 2 ** max_depth
    leaf = node - first_leaf
    cnt = torch.zeros(n_leaves, device=dev).scatter_add_(
        0, leaf, torch.ones_like(resid))
    s = torch.zeros(n_leaves, device=dev).scatter_add_(0, leaf, resid)
    values = (s / (cnt + lam)).tolist()
    return GBTree(max_depth, feature, threshold, values, cat_mask)


def _build_tree_sparse(sb: SparseBins, resid: torch.Tensor, num_bins: int,
                       max_depth: int, lam: float,
                       feature_types: Optional[torch.Tensor]) -> GBTree:
    """build_tree over a SparseBins: per level K10s over the batch's present
    features, K10b on that [n_nodes, nf, nb] histogram, the winner mapped
    back through feat_ids, and routing by bin lookup. A feature absent from
    the batch has one populated bin and so no valid candidate: leaving it
    out changes no winner, and feat_ids ascending keeps the lowest-feature
    tie rule. Without feature types the types are zeros and the tree has
    cat_mask = None, as the dense builder's."""
    B = sb.shape[0]
    dev = sb.device
    ids = sb.feat_ids.long()
    nf = ids.shape[0]
    if feature_types is None:
        ftype = torch.zeros(nf, dtype=torch.int32, device=dev)
    else:
        ftype = feature_types.to(device=dev, dtype=torch.int32)[ids]
    node = torch.zeros(B, dtype=torch.int64, device=dev)
    feature: List[int] = []
    threshold: List[int] = []
    cat_mask: List[int] = []
    for level in range(max_depth):
        first = 2 ** level - 1
        n_nodes = 2 ** level
        local = node - first
        if nf == 0:
            feat = torch.zeros(n_nodes, dtype=torch.int64, device=dev)
            thr, mask = feat - 1, feat.clone()
        else:
            cnt, s = ops.gbt_hist_sparse(
                sb.feat_ptr, sb.feat_row, sb.feat_bin, sb.feat_idx,
                sb.zero_bin, resid, local, n_nodes, num_bins)
            feat, thr, mask, _ = ops.gbt_best_split(cnt, s, ftype, lam)
            thr = thr.long()
            # a no-split node reports feature 0, as the dense builder does
            feat = torch.where(thr == -1, torch.zeros_like(thr),
                               ids[feat.long()])
        f_l, t_l, m_l = torch.stack([feat, thr, mask]).tolist()
        feature += f_l
        threshold += t_l
        cat_mask += m_l
        go_right = _route_right(sb.bin_of(feat[local]), thr[local],
                                mask[local])
        node = node * 2 + 1 + go_right.long()
    first_leaf = 2 ** max_depth - 1
    n_leaves = 2 ** max_depth
    leaf = node - first_leaf
    cnt = torch.zeros(n_leaves, device=dev).scatter_add_(
        0, leaf, torch.ones_like(resid))
    s = torch.zeros(n_leaves, device=dev).scatter_add_(0, leaf, resid)
    values = (s / (cnt + lam)).tolist()
    return GBTree(max_depth, feature, threshold, values,
                  cat_mask if feature_types is not None else None)


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
        done, last, pred = self._pred_cache.get(id(self.batch),
                                                (0, None, None))
        # valid only if the cached prefix is literally this forest's prefix
        # (offline eval may reload an older/replaced forest into the table)
        if pred is None or done > len(self.forest) or (
                done > 0 and self.forest[done - 1] is not last):
            done, pred = 0, torch.zeros_like(y)
        for t in self.forest[done:]:
            pred = pred + a["step_size"] * t.predict_bins(bins)
        self._pred_cache[id(self.batch)] = (
            len(self.forest), self.forest[-1] if self.forest else None, pred)
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
            key = (id(self.batch), c)
            done, last, pred = self._mc_cache.get(key, (0, None, None))
            forest = self.forests[c]
            if pred is None or done > len(forest) or (
                    done > 0 and forest[done - 1] is not last):
                done, pred = 0, torch.zeros_like(target)
            for t in forest[done:]:
                pred = pred + a["step_size"] * t.predict_bins(bins)
            self._mc_cache[key] = (len(forest),
                                   forest[-1] if forest else None, pred)
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

    def num_batch_examples(self) -> int:
        return self.batch[0].shape[0]


def _is_sparse(a: dict) -> bool:
    return str(a.get("sparse", "")).lower() in ("true", "1")


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
        n = y.shape[0]
        # torch.chunk's row ranges, so block i holds the rows the dense
        # branch would give it
        size = -(-n // n_blocks) if n else 0
        for lo in range(0, max(1, n), max(1, size)):
            hi = min(n, lo + size)
            e0, e1 = int(row_ptr[lo]), int(row_ptr[hi])
            x = SparseBins((row_ptr[lo:hi + 1] - e0, col[e0:e1], val[e0:e1],
                            F), nb, ftypes)
            blocks.append((x.to(device), y[lo:hi].float().to(device)))
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
        keep = torch.ones((B, k), dtype=torch.bool)
        keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
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
        row_ptr = torch.zeros(B + 1, dtype=torch.int64)
        row_ptr[1:] = torch.cumsum(keep.sum(dim=1), 0)
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


def build(job: JobConfig, ctx, cp):
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
    def _reslice(b, frac):
        # frac<=0 -> EMPTY batch: a stopped worker (StopWorkerOp) does
        # zero work and its sparse pulls/pushes carry zero keys
        n = 0 if frac <= 0 else max(1, int(b[0].shape[0] * frac))
        x = b[0].prefix(n) if isinstance(b[0], SparseBins) else b[0][:n]
        return (x, b[1][:n])

    provider = TrainingDataProvider(reslice=_reslice, local_blocks=
        make_batches(job, ctx.rank, ctx.device, ctx.world_size))
    return {MODEL_TABLE: table}, trainer, provider
