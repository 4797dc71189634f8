"""The BSP graph engine.

Reference mapping:
  * vertex table (Long -> Vertex<V,E>)      -> dense Table of vertex values;
    the adjacency (CSR over the LOCAL vertex partition) is device-resident
    per rank, like the reference's vertex edges living with the vertex.
  * two message tables, double-buffered     -> two dense Tables with a
    combiner update function ("add" for sum-combiners, "min" for min-
    combiners) — a message send IS a combining scatter on the owner
    (reference MessageManager.addMessage with MessageCombiner:92, flip:72).
  * superstep control (SuperstepResultMsg / SuperstepControlMsg,
    WorkerMsgManager.java:62-90)            -> an all-reduce of
    {num_active, msgs_sent} votes; the job halts when all vertices halted
    and no messages are in flight (PregelMaster.java:48-56).

The Computation SPI is vectorized MI355X-first: compute() transforms the
whole local vertex partition at once (values tensor + combined incoming
messages) instead of a per-vertex callable — per-vertex Java iteration
(ComputationCallable.java:36) would serialize the GPU.
"""

from __future__ import annotations

import time
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch
import torch.distributed as dist

from harmony_amd.config import JobConfig, TableConfig
from harmony_amd.et.table import Table
from harmony_amd.runtime.control import ControlPlane, TaskUnitScheduler


class Computation:
    """Vectorized vertex program (reference graph/api/Computation.java:25).

    All tensors are the LOCAL partition (rows = local vertices, aligned with
    the vertex table's local shard)."""

    # message-combiner semantics: "add" (sum) or "min"
    combiner = "add"
    # identity element written into the cleared message buffer
    msg_identity = 0.0
    msg_dim = 1

    def compute(self, superstep: int, values: torch.Tensor,
                incoming: torch.Tensor, has_msg: torch.Tensor, graph
                ) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor]:
        """Returns (new_values, per_edge_messages or None, active_mask).
        per_edge_messages: [num_local_edges, msg_dim] — message sent along
        each outgoing edge of the local CSR (dst = graph.edge_dst)."""
        raise NotImplementedError

    # Optional per-VERTEX form of compute() for the fused engine path
    # (PregelEngine(fused=True)): every out-edge of a vertex carries the
    # same value, so the engine needs one message per vertex and fans it
    # out through the pull index instead of a [num_local_edges] tensor.
    # edge_op says what an edge does to it: "copy" (message as is) or
    # "add_weight" (message + the edge's weight).
    edge_op = "copy"

    def vertex_messages(self, superstep: int, values: torch.Tensor,
                        incoming: torch.Tensor, has_msg: torch.Tensor, graph
                        ) -> Tuple[torch.Tensor, Optional[torch.Tensor],
                                   Optional[torch.Tensor], torch.Tensor]:
        """Returns (new_values, vert_msg or None, send_mask or None,
        active_mask). vert_msg: [n_local] float32, the value each vertex
        sends along all its out-edges (None: nobody sends); send_mask:
        [n_local] bool, the vertices that send (None: all of them)."""
        raise NotImplementedError

    def has_vertex_messages(self) -> bool:
        return (type(self).vertex_messages
                is not Computation.vertex_messages)


@dataclass
class LocalGraph:
    """CSR adjacency of the local vertex partition."""

    vertex_lo: int                 # first global vertex id owned locally
    row_ptr: torch.Tensor          # [n_local+1]
    edge_dst: torch.Tensor         # [n_local_edges] global dst ids
    out_degree: torch.Tensor       # [n_local]
    num_vertices_global: int
    # per-edge values (reference Vertex<V,E> / DefaultEdge), aligned with
    # edge_dst; None for graphs without edge values
    edge_weight: Optional[torch.Tensor] = None   # [n_local_edges] float32


@dataclass
class PullIndex:
    """The local edge list inverted once: for each destination row, the
    local sources that send to it (see build_pull_index)."""

    n_local: int
    in_ptr: torch.Tensor           # int64 [R+1], R = n_local + U
    in_src: torch.Tensor           # int32 [Ein] local source vertex index
    in_w: Optional[torch.Tensor]   # float32 [Ein] or None
    remote_keys: torch.Tensor      # int64 [U] global ids of rows >= n_local
    # destination row of every local edge in original edge order; kept only
    # on request, for build_push_index, which takes it over
    row_of_edge: Optional[torch.Tensor] = None   # int64 [E]

    @property
    def num_rows(self) -> int:
        return int(self.in_ptr.shape[0]) - 1


@dataclass
class PushIndex:
    """The local out-CSR with every destination renamed to its row in the
    pull index's row space (see build_push_index)."""

    out_ptr: torch.Tensor          # int64 [n_local+1]
    out_row: torch.Tensor          # int32 [E] row in 0..R-1, edge order
    out_w: Optional[torch.Tensor]  # float32 [E] or None


def build_pull_index(graph: LocalGraph, msg_table: Table,
                     keep_rows: bool = False) -> PullIndex:
    """Invert the local CSR into a pull index for ops.pregel_pull.

    Rows 0..n_local-1 are the local vertices in shard order (a vertex
    without in-edges keeps an empty range); rows n_local..n_local+U-1 are
    the U distinct destinations of local edges that another rank owns, in
    ascending key order (`remote_keys`). A stable sort keeps every row's
    sources in original edge order, which fixes the summation order.

    The index is tied to `msg_table`'s ownership at the time of the call:
    which destinations are local rows and which are remote is baked in.
    Pregel tables do not migrate mid-run, so it is built once per job in
    PregelEngine.set_graph. keep_rows leaves the per-edge destination rows
    on the index for build_push_index."""
    dev = graph.edge_dst.device
    n_local = int(graph.row_ptr.shape[0]) - 1
    n_edges = int(graph.edge_dst.shape[0])
    if n_local >= 2 ** 31 or n_edges >= 2 ** 31:
        raise ValueError(
            f"pull index needs n_local ({n_local}) and the local edge count "
            f"({n_edges}) below 2^31: in_src and the kernel's source index "
            "are int32")
    dst = graph.edge_dst.to(torch.int64)
    counts = graph.row_ptr[1:] - graph.row_ptr[:-1]
    src_local = torch.repeat_interleave(
        torch.arange(n_local, dtype=torch.int64, device=dev), counts)
    owner = msg_table.ownership.owner.to(dev)[msg_table.part.block_of(dst)]
    is_local = owner == msg_table.rank
    row_of_edge = torch.empty(n_edges, dtype=torch.int64, device=dev)
    local_rows = msg_table.local_rows_of(dst[is_local])
    if local_rows.numel() and int(local_rows.max()) >= n_local:
        raise ValueError("a locally owned destination lies outside the "
                         "local vertex range the graph was built for")
    row_of_edge[is_local] = local_rows
    remote_keys, inv = torch.unique(dst[~is_local], return_inverse=True)
    row_of_edge[~is_local] = n_local + inv
    num_rows = n_local + int(remote_keys.shape[0])
    order = torch.argsort(row_of_edge, stable=True)
    in_ptr = torch.zeros(num_rows + 1, dtype=torch.int64, device=dev)
    in_ptr[1:] = torch.cumsum(
        torch.bincount(row_of_edge, minlength=num_rows), 0)
    in_w = None
    if graph.edge_weight is not None:
        in_w = graph.edge_weight.to(torch.float32)[order].contiguous()
    return PullIndex(n_local=n_local, in_ptr=in_ptr,
                     in_src=src_local[order].to(torch.int32).contiguous(),
                     in_w=in_w, remote_keys=remote_keys,
                     row_of_edge=row_of_edge if keep_rows else None)


def build_push_index(graph: LocalGraph, pull_index: PullIndex,
                     msg_table: Table) -> PushIndex:
    """The out-edge view of the same edge list for ops.pregel_push: the
    graph's own CSR with out_row[e] = the pull index's row of edge e's
    destination, so push and pull write the same [R] result and everything
    after the op is shared.

    The rows are the ones build_pull_index(keep_rows=True) computed while
    numbering the remote destinations; they are taken over from
    `pull_index` (and dropped there), not derived a second time, so the two
    indexes cannot disagree. out_w is graph.edge_weight itself."""
    rows = pull_index.row_of_edge
    if rows is None:
        raise ValueError("build_push_index needs a pull index built with "
                         "keep_rows=True (its row_of_edge)")
    if pull_index.num_rows >= 2 ** 31:
        raise ValueError(
            f"push index needs fewer than 2^31 rows, got "
            f"{pull_index.num_rows}: out_row is int32")
    pull_index.row_of_edge = None
    out_w = graph.edge_weight
    if out_w is not None and out_w.dtype != torch.float32:
        out_w = out_w.to(torch.float32)
    return PushIndex(out_ptr=graph.row_ptr.to(torch.int64).contiguous(),
                     out_row=rows.to(torch.int32).contiguous(), out_w=out_w)


# Default share of the local edges below which direction="auto" pushes.
# Measured (scripts/pregel_push_ab.py, profiles/pregel_push_ab.md): on the
# ring+random graph at 2^20 x 8 push, as the engine calls it, is no slower
# than pull up to a share of 2^-4 of the edges, at 2^20 x 64 up to 2^-3;
# the largest power of two that holds on both is 2^-4, halved once as a
# margin because the crossover moves with degree and skew.
DEFAULT_PUSH_THRESHOLD = 2.0 ** -5

DIRECTIONS = ("pull", "push", "auto")


class PregelEngine:
    """BSP engine; see the module docstring.

    fused=True sends and combines through ops.pregel_pull (K13) over the
    pull index. `direction` chooses, for the fused path, which way a
    superstep's messages travel:
      "pull"  K13 over every in-edge of every row (the default);
      "push"  K13p (ops.pregel_push) along the out-edges of the sending
              vertices only; min combiner only;
      "auto"  per rank and per superstep: push iff the out-degrees of the
              sending vertices sum to less than push_threshold *
              num_local_edges (strictly, so an empty frontier pushes, a
              no-op), else pull. With the add combiner, or when everyone
              sends (send_mask None), auto pulls.
    Both ops give the same [R] result value for value, and everything after
    them (local rows, remote rows, the vote, the one collective) is shared,
    so ranks need not agree on the direction. push_supersteps and
    pull_supersteps count the supersteps of the last run() that used each.

    push_threshold defaults to DEFAULT_PUSH_THRESHOLD = 2^-5: the largest
    power-of-two share at which push was measured no slower than pull on
    both 2^20 x 8 and 2^20 x 64 (2^-4), halved once as a margin
    (profiles/pregel_push_ab.md). "pull" and "push" add no host read to a
    superstep; "auto" adds one, of the frontier's edge count. That read
    costs more than the kernel saves where a superstep is bound by host
    launches (low degree, high diameter), so "pull" stays the default."""

    def __init__(self, job: JobConfig, comp: Computation, num_vertices: int,
                 ctx, cp: ControlPlane, tus: Optional[TaskUnitScheduler] = None,
                 max_supersteps: int = 100, fused: bool = False,
                 direction: str = "pull",
                 push_threshold: Optional[float] = None):
        self.job = job
        self.comp = comp
        if direction not in DIRECTIONS:
            raise ValueError(f"direction must be one of {DIRECTIONS}, "
                             f"got {direction!r}")
        if direction != "pull" and not fused:
            raise ValueError(f"direction={direction!r} needs fused=True: "
                             "the unfused path sends per-edge messages")
        if direction == "push" and comp.combiner != "min":
            raise ValueError(
                "direction='push' supports the min combiner only, this "
                f"computation combines with {comp.combiner!r}")
        self.direction = direction
        self.push_threshold = float(DEFAULT_PUSH_THRESHOLD
                                    if push_threshold is None
                                    else push_threshold)
        self.push: Optional[PushIndex] = None
        self.push_supersteps = 0
        self.pull_supersteps = 0
        # fused: send + combine through the pull index (ops.pregel_pull,
        # K13) instead of per-edge messages + a combining scatter
        self.fused = bool(fused)
        if self.fused and (comp.msg_dim != 1
                           or not comp.has_vertex_messages()):
            raise ValueError(
                "fused=True needs msg_dim == 1 and a Computation that "
                "implements vertex_messages()")
        self.pull: Optional[PullIndex] = None
        self.graph: Optional[LocalGraph] = None   # set_graph() after tables
        self.ctx = ctx
        self.cp = cp
        self.tus = tus or TaskUnitScheduler(cp, {job.job_id})
        self.max_supersteps = max_supersteps
        n = num_vertices
        mk = lambda name, init: Table(  # noqa: E731
            TableConfig(table_id=f"{job.job_id}/{name}", num_keys=n,
                        value_dim=comp.msg_dim, dtype="float32",
                        num_blocks=max(ctx.world_size, min(256, n)),
                        update_fn=comp.combiner, init_fn="zeros"),
            ctx.rank, ctx.world_size, ctx.device, comm=ctx.new_data_plane())
        self.vertex_table = Table(
            TableConfig(table_id=f"{job.job_id}/vertex", num_keys=n,
                        value_dim=comp.msg_dim, dtype="float32",
                        num_blocks=max(ctx.world_size, min(256, n)),
                        update_fn="assign", init_fn="zeros"),
            ctx.rank, ctx.world_size, ctx.device, comm=ctx.new_data_plane())
        # double-buffered message tables (reference PregelJobEntity creates
        # vertex + msg1 + msg2)
        self.msg = [mk("msg1", None), mk("msg2", None)]
        self._has = [None, None]   # has-message masks (local rows)
        self.cur = 0
        self._phase = 0
        self.supersteps_run = 0

    def local_vertex_range(self):
        """Global key range of this rank's vertex partition (the graph the
        caller builds must cover exactly this range)."""
        bs = self.vertex_table.block_size
        owned = self.vertex_table.owned_blocks
        lo = owned[0] * bs if owned else 0
        hi = min((owned[-1] + 1) * bs,
                 self.vertex_table.cfg.num_keys) if owned else 0
        return lo, hi

    def set_graph(self, graph: LocalGraph) -> None:
        self.graph = graph
        if self.fused:
            # both message tables share one layout; see build_pull_index
            # for why the index is valid for the whole run
            can_push = (self.direction != "pull"
                        and self.comp.combiner == "min")
            self.pull = build_pull_index(graph, self.msg[0],
                                         keep_rows=can_push)
            if can_push:
                self.push = build_push_index(graph, self.pull, self.msg[0])
                self._out_deg = (self.push.out_ptr[1:]
                                 - self.push.out_ptr[:-1])
                self._everyone = torch.arange(
                    self.pull.n_local, dtype=torch.int32,
                    device=self.push.out_ptr.device)

    def _next_phase(self):
        self._phase += 1
        return self._phase

    def _local_slice(self, table: Table) -> torch.Tensor:
        return table.shard

    def _clear(self, table: Table, identity: float) -> None:
        table.shard.fill_(identity)

    def run(self) -> torch.Tensor:
        """Run supersteps to halt; returns final local vertex values."""
        if self.fused:
            return self._run_fused()
        comp, g = self.comp, self.graph
        dev = self.ctx.device
        n_local = g.row_ptr.shape[0] - 1
        values = self.vertex_table.shard[:n_local]
        ident = comp.msg_identity
        for t in self.msg:
            self._clear(t, ident)
        has_msg = torch.zeros(n_local, dtype=torch.bool, device=dev)
        active = torch.ones(n_local, dtype=torch.bool, device=dev)
        jid = self.job.job_id
        zero_keys = torch.empty(0, dtype=torch.int64, device=dev)
        zero_msgs = torch.empty((0, comp.msg_dim), dtype=torch.float32,
                                device=dev)
        lo, _hi = self.local_vertex_range()
        for step in range(self.max_supersteps):
            self.supersteps_run = step + 1
            # COMP: local vertex update over combined incoming messages
            incoming = self.msg[self.cur].shard[:n_local]
            values, edge_msgs, active = comp.compute(
                step, values, incoming, has_msg, g)
            # clear the consumed buffer for reuse (flip semantics,
            # reference MessageManager.flip:72-74)
            self._clear(self.msg[self.cur], ident)
            # SEND + SYNC fused: ONE collective per superstep. Every rank
            # enters the push even with zero messages (a per-rank skip
            # would strand peers inside the collective); the halt vote
            # (allVerticesHalt AND noOngoingMsgs, PregelMaster.java:48-56)
            # rides the push's count exchange as a piggyback sum, and the
            # data legs are skipped symmetrically when no rank sent.
            nxt = self.msg[1 - self.cur]
            keys = (g.edge_dst if edge_msgs is not None else zero_keys)
            msgs = (edge_msgs if edge_msgs is not None else zero_msgs)
            sent = int(keys.numel())
            nxt.last_touched_keys = None
            vote = torch.tensor([int(active.sum()), sent])
            with self.tus.net(jid, self._next_phase()):
                sums = nxt.update(keys, msgs, piggyback=vote)
            self.cur = 1 - self.cur
            # incremental has-message mask from the owner-apply's touched
            # keys (replaces the full-shard != identity scan)
            has_msg = torch.zeros(n_local, dtype=torch.bool, device=dev)
            touched = getattr(self.msg[self.cur], "last_touched_keys", None)
            if touched is not None and touched.numel():
                rows = self.msg[self.cur].local_rows_of(touched.to(dev))
                has_msg[rows[rows < n_local]] = True
            if sums is not None and int(sums[0]) == 0 and int(sums[1]) == 0:
                break
        self.vertex_table.shard[:n_local] = values
        return values

    def _push_or_pull(self, send_mask: Optional[torch.Tensor]):
        """This superstep's direction: (True, the frontier's edge count or
        -1) to push, (False, -1) to pull. "pull" and "push" cost no host
        read (K13p takes the mask itself, over the frontier of all
        vertices); "auto" costs one, of the frontier's edge count."""
        if self.push is None:          # "pull", or "auto" with add
            return False, -1
        if self.direction == "push":
            return True, -1
        if send_mask is None:          # everyone sends
            return False, -1
        edges = int((self._out_deg * send_mask).sum())
        if edges < self.push_threshold * self.push.out_row.shape[0]:
            return True, edges
        return False, -1

    def _run_fused(self) -> torch.Tensor:
        """run() with send + combine as ONE gather-reduce per superstep
        (K13): no per-edge message tensor, no per-superstep sort. Local
        destinations are written straight into the next message shard;
        only the combined values of remote destinations go through the
        push, which every rank still enters once per superstep."""
        from harmony_amd import ops

        comp, g, pull = self.comp, self.graph, self.pull
        dev = self.ctx.device
        n_local = pull.n_local
        n_remote = int(pull.remote_keys.shape[0])
        values = self.vertex_table.shard[:n_local]
        ident = comp.msg_identity
        for t in self.msg:
            self._clear(t, ident)
        has_msg = torch.zeros(n_local, dtype=torch.bool, device=dev)
        jid = self.job.job_id
        zero_keys = torch.empty(0, dtype=torch.int64, device=dev)
        zero_msgs = torch.empty((0, 1), dtype=torch.float32, device=dev)
        add_weight = comp.edge_op == "add_weight"
        w_const = float(getattr(comp, "edge_weight", 0.0))
        self.push_supersteps = self.pull_supersteps = 0
        for step in range(self.max_supersteps):
            self.supersteps_run = step + 1
            incoming = self.msg[self.cur].shard[:n_local]
            values, vert_msg, send_mask, active = comp.vertex_messages(
                step, values, incoming, has_msg, g)
            self._clear(self.msg[self.cur], ident)
            nxt = self.msg[1 - self.cur]
            nxt.last_touched_keys = None
            keys, msgs = zero_keys, zero_msgs
            has_msg = torch.zeros(n_local, dtype=torch.bool, device=dev)
            n_active = active.sum()
            if vert_msg is None:
                vote = torch.stack([n_active, torch.zeros_like(n_active)])
            else:
                pushing, hint = self._push_or_pull(send_mask)
                if pushing:
                    self.push_supersteps += 1
                    out, flag = ops.pregel_push(
                        self.push.out_ptr, self.push.out_row,
                        self.push.out_w, w_const,
                        vert_msg.to(torch.float32), self._everyone,
                        pull.num_rows, comp.combiner, add_weight,
                        send_mask=send_mask, _edges_hint=hint)
                else:
                    self.pull_supersteps += 1
                    out, flag = ops.pregel_pull(
                        pull.in_ptr, pull.in_src, pull.in_w, w_const,
                        vert_msg.to(torch.float32), send_mask,
                        comp.combiner, add_weight)
                # local rows first: unflagged rows hold the identity, like
                # the cleared shard, and the push below combines remote
                # ranks' contributions on top of them
                nxt.shard[:n_local, 0] = out[:n_local]
                has_msg = flag[:n_local].bool()
                if n_remote:
                    sel = flag[n_local:].bool()
                    keys = pull.remote_keys[sel]
                    msgs = out[n_local:][sel].unsqueeze(1)
                vote = torch.stack([n_active, flag.sum()])
            vote = vote.to("cpu", torch.int64)
            with self.tus.net(jid, self._next_phase()):
                sums = nxt.update(keys, msgs, assume_unique=True,
                                  piggyback=vote)
            self.cur = 1 - self.cur
            touched = getattr(self.msg[self.cur], "last_touched_keys", None)
            if touched is not None and touched.numel():
                rows = self.msg[self.cur].local_rows_of(touched.to(dev))
                has_msg[rows[rows < n_local]] = True
            if sums is not None and int(sums[0]) == 0 and int(sums[1]) == 0:
                break
        self.vertex_table.shard[:n_local] = values
        return values
