"""The elastic table: GPU-resident sharded key-value storage.

Reference: et/evaluator/impl/TableImpl.java:44 (user-facing op routing),
TabletImpl/BlockStore/BlockImpl (local block storage), evaluator/api/Table.java:35.

MI355X-native design, deliberately not a translation:

* The reference stores each block as a ConcurrentHashMap<K,V> of boxed Java
  vectors and routes every op through per-block comm-thread queues
  (CommManager.java:36). Here a table over a dense integer keyspace stores all
  locally-owned blocks in ONE contiguous device tensor (`shard`,
  [n_owned_blocks * block_size, value_dim]) resident in the GPU's 288 GB HBM3E.
  Multi-key get/update on local rows is a single index_select / index-reduce
  kernel; remote multi-key ops become RCCL collectives over xGMI (et/comm.py)
  instead of Avro RPC.
* get_or_init == get: the shard is fully initialized at creation by the
  table's deterministic per-key init function, which matches the reference's
  UpdateFunction.initValue semantics without a per-access existence check.
* "Object tables" (host-side dict blocks) cover non-tensor values such as
  GBT's label -> list-of-trees (reference gbt/GBTETModelUpdateFunction.java:32).
"""

from __future__ import annotations

from typing import Any, Callable, Dict, List, Optional

import torch

from harmony_amd.config import TableConfig, dtype_of
from harmony_amd import ops
from harmony_amd.et import update_functions as uf
from harmony_amd.et.ownership import Ownership
from harmony_amd.et.partitioner import HashBasedPartitioner, OrderingBasedPartitioner


class Table:
    """Dense tensor-backed elastic table shard on one executor (rank)."""

    def __init__(self, cfg: TableConfig, rank: int, world_size: int,
                 device: torch.device, comm=None,
                 ownership: Optional[Ownership] = None):
        assert cfg.storage == "dense"
        self.cfg = cfg
        self.rank = rank
        self.world_size = world_size
        self.device = device
        self.comm = comm  # et.comm.DataPlane or None (single-process/local)
        self.dtype = dtype_of(cfg.dtype)
        self.part = OrderingBasedPartitioner(cfg.num_keys, cfg.num_blocks)
        self.block_size = self.part.block_size
        self.ownership = ownership or Ownership(cfg.num_blocks, world_size)
        self.shard: torch.Tensor = torch.empty(0)
        self._block_slot: torch.Tensor = torch.empty(0)  # [num_blocks] int64, -1 if remote
        self._alloc_shard()

    # ------------------------------------------------------------------ setup

    def _alloc_shard(self) -> None:
        owned = self.ownership.owned_blocks(self.rank)
        # Local data placement, tracked separately from the ownership map:
        # during ownership-first migration the two are transiently different
        # (owner flips before data moves — reference MigrationExecutor.java:134).
        self._local_blocks: List[int] = list(owned)
        init = uf.init_fn(self.cfg.init_fn)
        # Deterministic per-block init: seed derived from (table, block) so a
        # key's initial value is identical regardless of which rank owns it
        # (needed for elastic migration + restart reproducibility).
        rows = []
        for b in owned:
            t = init((self.block_size, self.cfg.value_dim), self.dtype, self.device,
                     seed=_block_seed(self.cfg.table_id, b), **self.cfg.init_args)
            rows.append(t)
        if rows:
            self.shard = torch.cat(rows, dim=0)
        else:
            self.shard = torch.empty((0, self.cfg.value_dim), dtype=self.dtype,
                                     device=self.device)
        self._buf = self.shard     # capacity buffer (see _rebuild)
        slot = torch.full((self.cfg.num_blocks,), -1, dtype=torch.int64)
        for i, b in enumerate(owned):
            slot[b] = i
        self._block_slot = slot.to(self.device)

    def init_block_tensor(self, block_id: int) -> torch.Tensor:
        """Freshly initialized values of one block (used by migration targets)."""
        init = uf.init_fn(self.cfg.init_fn)
        return init((self.block_size, self.cfg.value_dim), self.dtype, self.device,
                    seed=_block_seed(self.cfg.table_id, block_id), **self.cfg.init_args)

    # ------------------------------------------------------------- local view

    @property
    def owned_blocks(self) -> List[int]:
        """Blocks whose data is locally resident (sorted)."""
        return self._local_blocks

    def num_local_rows(self) -> int:
        return self.shard.shape[0]

    def local_block_view(self, block_id: int) -> torch.Tensor:
        slot = int(self._block_slot[block_id])
        assert slot >= 0, f"block {block_id} not owned by rank {self.rank}"
        return self.shard[slot * self.block_size:(slot + 1) * self.block_size]

    def local_rows_of(self, keys: torch.Tensor) -> torch.Tensor:
        """Map (locally-owned) keys to row indices in `shard`."""
        blocks = self.part.block_of(keys)
        slots = self._block_slot[blocks]
        return slots * self.block_size + self.part.offset_in_block(keys)

    # ------------------------------------------------------ single-rank ops

    def get_local(self, keys: torch.Tensor) -> torch.Tensor:
        return self.shard[self.local_rows_of(keys)]

    def put_local(self, keys: torch.Tensor, values: torch.Tensor) -> None:
        self.shard[self.local_rows_of(keys)] = values.to(self.dtype)

    def update_local(self, keys: torch.Tensor, deltas: torch.Tensor) -> None:
        """Apply the table's update function to aggregated per-key deltas.

        Keys MUST be unique (aggregate first with ops.segment_sum); the update
        function runs once per key, matching the reference's per-update apply
        after multiUpdate merging (TableImpl.java:460, BlockImpl.update:71).
        """
        rows = self.local_rows_of(keys)
        # incremental touched-row tracking (Pregel has_msg; reset by callers)
        self.last_touched_keys = keys
        if self.device.type == "cuda" and ops.fused_apply_supported(self.cfg.update_fn):
            # fused gather-apply-scatter kernel (K3/K9)
            ops.scatter_apply(self.shard, rows, deltas.to(self.dtype),
                              self.cfg.update_fn,
                              *uf.fused_apply_args(self.cfg.update_fn,
                                                   self.cfg.update_args))
            return
        fn = uf.update_fn(self.cfg.update_fn)
        vals = self.shard[rows]
        self.shard[rows] = fn(vals, deltas.to(vals.dtype), **self.cfg.update_args)

    def apply_update_dense_local(self, agg_delta: torch.Tensor) -> None:
        """Update the whole local shard with an aggregated dense delta
        (the fused epilogue of a reduce-scatter push)."""
        if self.device.type == "cuda" and ops.fused_apply_supported(self.cfg.update_fn):
            ops.dense_apply(self.shard, agg_delta.to(self.dtype),
                            self.cfg.update_fn,
                            *uf.fused_apply_args(self.cfg.update_fn,
                                                 self.cfg.update_args))
            return
        fn = uf.update_fn(self.cfg.update_fn)
        fn(self.shard, agg_delta.to(self.shard.dtype), **self.cfg.update_args)

    # -------------------------------------------------------- distributed ops

    def _local_only(self) -> bool:
        return self.comm is None or self.world_size == 1

    def get(self, keys: torch.Tensor) -> torch.Tensor:
        """multiGet/multiGetOrInit (reference TableImpl.java:284,366)."""
        if self._local_only():
            return self.get_local(keys)
        return self.comm.pull_keys(self, keys)

    # get_or_init is get: the shard is always fully initialized.
    get_or_init = get

    def put(self, keys: torch.Tensor, values: torch.Tensor) -> None:
        """multiPut (reference TableImpl.java:156): overwrite values at the
        owners (no update function)."""
        if self._local_only():
            self.put_local(keys, values)
            return
        self.comm.put_keys(self, keys, values)

    def remove(self, keys: torch.Tensor) -> None:
        """multiRemove (reference TableImpl.java:513). Dense tables have a
        value for every key by construction, so remove restores the
        deterministic initial value (the state a fresh getOrInit would see —
        observationally the reference's remove-then-getOrInit)."""
        if self._local_only():
            self.remove_local(keys)
            return
        self.comm.remove_keys(self, keys)

    def remove_local(self, keys: torch.Tensor) -> None:
        keys = keys.to(self.device, torch.int64)
        rows = self.local_rows_of(keys)
        blocks = self.part.block_of(keys)
        init = uf.init_fn(self.cfg.init_fn)
        # regenerate per-block init rows and scatter the removed offsets
        for b in torch.unique(blocks).tolist():
            fresh = self.init_block_tensor(int(b))
            sel = blocks == b
            offs = self.part.offset_in_block(keys[sel])
            self.shard[rows[sel]] = fresh[offs]

    def update(self, keys: torch.Tensor, deltas: torch.Tensor,
               assume_unique: bool = False, piggyback=None):
        """multiUpdate (reference TableImpl.java:460): route deltas to owner
        ranks; the owner applies the table's update function.
        assume_unique: keys are already unique + per-key aggregated (skips a
        device sort/unique on the hot path). piggyback: small int vector
        summed globally inside the push's count exchange (see
        DataPlane.push_keys); returned when given."""
        if self._local_only():
            if keys.numel():
                if not assume_unique:
                    keys, deltas = uf.merge_key_deltas(keys, deltas,
                                                       self.cfg.update_fn)
                self.update_local(keys, deltas)
            return piggyback
        return self.comm.push_keys(self, keys, deltas,
                                   assume_unique=assume_unique,
                                   piggyback=piggyback)

    def pull_all(self) -> torch.Tensor:
        """Gather the whole table (dense apps pull every partition each batch,
        reference MLRTrainer.java:185-187) -> [padded_num_keys, value_dim]."""
        if self._local_only():
            return self.shard
        return self.comm.pull_all(self)

    def push_dense(self, grad_full: torch.Tensor) -> None:
        """Dense push of a full-table delta: reduce-scatter + fused update."""
        if self._local_only():
            self.apply_update_dense_local(grad_full)
            return
        self.comm.push_dense(self, grad_full)

    # ------------------------------------------------------------ migration

    def drop_blocks(self, block_ids: List[int]) -> Dict[int, torch.Tensor]:
        """Remove blocks from the local shard; returns their data (for the
        migration sender). Ownership must be updated separately."""
        out = {b: self.local_block_view(b).clone() for b in block_ids}
        keep = [b for b in self._local_blocks if b not in set(block_ids)]
        self._rebuild(keep, carry={})
        return out

    def adopt_blocks(self, blocks: Dict[int, torch.Tensor]) -> None:
        """Insert received blocks into the local shard."""
        self._rebuild(sorted(set(self._local_blocks) | set(blocks)), carry=blocks)

    def _rebuild(self, new_block_list: List[int],
                 carry: Dict[int, torch.Tensor]) -> None:
        """Re-lay the shard for a new block list. IN PLACE whenever the
        capacity buffer fits (transient memory = ONE block, not a full
        shard copy — round 1 concatenated a second full shard, 2x peak at
        100+ GB scale); a capacity miss reallocates once with headroom so
        steady-state migration churn never reallocates again."""
        bs, vd = self.block_size, self.cfg.value_dim
        final = sorted(new_block_list)
        need = len(final) * bs
        buf = getattr(self, "_buf", None)
        if buf is None or buf.shape[0] < need or buf.device != self.device:
            # grow (or first migration): allocate with 25% block headroom
            cap = (len(final) + max(1, len(final) // 4)) * bs
            newbuf = torch.empty((cap, vd), dtype=self.dtype,
                                 device=self.device)
            for i, b in enumerate(final):
                src = (carry[b].to(self.device, self.dtype) if b in carry
                       else self.local_block_view(b))
                newbuf[i * bs:(i + 1) * bs] = src
            self._buf = newbuf
        else:
            # in-place: move kept blocks to their new slots. Downward moves
            # (dst < src) in increasing dst order, upward in decreasing dst
            # order — never clobbers an unmoved block; a one-block temp
            # covers the overlapping-src/dst case.
            moves = []
            for i, b in enumerate(final):
                if b in carry:
                    continue
                src = int(self._block_slot[b])
                if src != i:
                    moves.append((src, i))
            for src, dst in sorted([m for m in moves if m[1] < m[0]],
                                   key=lambda m: m[1]):
                self._block_move(buf, src, dst)
            for src, dst in sorted([m for m in moves if m[1] > m[0]],
                                   key=lambda m: -m[1]):
                self._block_move(buf, src, dst)
            for i, b in enumerate(final):
                if b in carry:
                    buf[i * bs:(i + 1) * bs] = carry[b].to(self.device,
                                                           self.dtype)
        self.shard = self._buf.narrow(0, 0, need)
        slot = torch.full((self.cfg.num_blocks,), -1, dtype=torch.int64)
        for i, b in enumerate(final):
            slot[b] = i
        self._block_slot = slot.to(self.device)
        self._local_blocks = final

    def _block_move(self, buf: torch.Tensor, src: int, dst: int) -> None:
        bs = self.block_size
        s = buf[src * bs:(src + 1) * bs]
        d = buf[dst * bs:(dst + 1) * bs]
        d.copy_(s)          # block-granular slots never overlap


class ObjectTable:
    """Host-side object-valued table (reference BlockImpl's map semantics) for
    values that are not fixed-width tensors (e.g. GBT's tree lists)."""

    def __init__(self, cfg: TableConfig, rank: int, world_size: int, comm=None,
                 ownership: Optional[Ownership] = None,
                 init_value: Callable[[int], Any] = lambda k: None,
                 update_value: Callable[[Any, Any], Any] = lambda v, d: d):
        assert cfg.storage == "object"
        self.cfg = cfg
        self.rank = rank
        self.world_size = world_size
        self.comm = comm
        self.part = (OrderingBasedPartitioner(cfg.num_keys, cfg.num_blocks)
                     if cfg.is_ordered else HashBasedPartitioner(cfg.num_blocks))
        self.ownership = ownership or Ownership(cfg.num_blocks, world_size)
        self.init_value = init_value
        self.update_value = update_value
        self.blocks: Dict[int, Dict[int, Any]] = {
            b: {} for b in self.ownership.owned_blocks(rank)}
        # bumped by out-of-band content changes (checkpoint reload,
        # migration, puts/removes) so replicated caches built from the
        # append-only push stream know to rebuild (gbt.py forest replica)
        self.content_epoch = 0

    def get_or_init_local(self, key: int) -> Any:
        b = self.part.block_of_int(key)
        blk = self.blocks[b]
        if key not in blk:
            blk[key] = self.init_value(key)
        return blk[key]

    def update_local(self, key: int, delta: Any) -> Any:
        b = self.part.block_of_int(key)
        blk = self.blocks[b]
        blk[key] = self.update_value(blk.get(key, self.init_value(key)), delta)
        return blk[key]

    def put_local(self, key: int, value: Any) -> None:
        self.content_epoch += 1
        self.blocks[self.part.block_of_int(key)][key] = value

    def remove_local(self, key: int) -> Any:
        self.content_epoch += 1
        return self.blocks[self.part.block_of_int(key)].pop(key, None)

    def get(self, key: int) -> Any:
        """Local get (single-rank); multi-rank apps use pull_all()."""
        return self.get_or_init_local(key)

    def update(self, key: int, delta: Any) -> None:
        """Local update (single-rank); multi-rank apps use push_items()."""
        self.update_local(key, delta)

    def pull_all(self) -> Dict[int, Any]:
        """Gather all key/values to every rank (collective)."""
        if self.comm is None or self.world_size == 1:
            out: Dict[int, Any] = {}
            for blk in self.blocks.values():
                out.update(blk)
            return out
        return self.comm.object_pull_all(self)

    def push_items(self, items) -> None:
        """Collective push of (key, delta) items; owners apply updates."""
        if self.comm is None or self.world_size == 1:
            for key, delta in items:
                self.update_local(key, delta)
            return
        self.comm.object_push(self, items)

    # migration support
    def drop_blocks(self, block_ids: List[int]) -> Dict[int, Dict[int, Any]]:
        self.content_epoch += 1
        return {b: self.blocks.pop(b) for b in block_ids}

    def adopt_blocks(self, blocks: Dict[int, Dict[int, Any]]) -> None:
        self.content_epoch += 1
        self.blocks.update(blocks)


def _block_seed(table_id: str, block_id: int) -> int:
    h = 2166136261
    for ch in table_id:
        h = ((h ^ ord(ch)) * 16777619) & 0xFFFFFFFF
    return (h * 31 + block_id) & 0x7FFFFFFF
