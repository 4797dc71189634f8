"""Graph apps: PageRank, single-source shortest path, connected components.

Reference: pregel/graphapps/pagerank (PagerankComputation + sum combiner)
and pregel/graphapps/shortestpath (min combiner); connected components
(min-label propagation) has no reference counterpart. All are vectorized
over the local vertex partition (see engine.Computation).
"""

from __future__ import annotations

import torch

from harmony_amd.pregel.engine import Computation, LocalGraph


class PageRankComputation(Computation):
    """val = 0.15/N + 0.85 * sum(in msgs); send val/out_deg along edges for
    `num_iters` supersteps (reference PagerankComputation)."""

    combiner = "add"
    msg_identity = 0.0
    msg_dim = 1
    edge_op = "copy"

    def __init__(self, num_iters: int = 20):
        self.num_iters = num_iters

    def compute(self, superstep, values, incoming, has_msg, graph: LocalGraph):
        n = graph.num_vertices_global
        if superstep == 0:
            new = torch.full_like(values, 1.0 / n)
        else:
            new = 0.15 / n + 0.85 * incoming
        if superstep >= self.num_iters:
            active = torch.zeros(values.shape[0], dtype=torch.bool,
                                 device=values.device)
            return new, None, active
        counts = graph.row_ptr[1:] - graph.row_ptr[:-1]
        contrib = new.squeeze(1) / graph.out_degree.clamp_min(1)
        edge_msgs = contrib.repeat_interleave(counts).unsqueeze(1)
        active = torch.ones(values.shape[0], dtype=torch.bool,
                            device=values.device)
        return new, edge_msgs, active

    def vertex_messages(self, superstep, values, incoming, has_msg,
                        graph: LocalGraph):
        """compute() with one message per vertex (every out-edge carries
        val/out_deg) — same arithmetic, no per-edge expansion."""
        n = graph.num_vertices_global
        if superstep == 0:
            new = torch.full_like(values, 1.0 / n)
        else:
            new = 0.15 / n + 0.85 * incoming
        if superstep >= self.num_iters:
            active = torch.zeros(values.shape[0], dtype=torch.bool,
                                 device=values.device)
            return new, None, None, active
        vert_msg = new.squeeze(1) / graph.out_degree.clamp_min(1)
        active = torch.ones(values.shape[0], dtype=torch.bool,
                            device=values.device)
        return new, vert_msg, None, active


class ShortestPathComputation(Computation):
    """Min-combiner relaxation: a vertex adopts the smallest incoming
    distance and, when improved, relaxes its out-edges (reference
    shortestpath app). Vertices halt immediately; messages wake them."""

    combiner = "min"
    msg_identity = float("inf")
    msg_dim = 1
    edge_op = "add_weight"

    def __init__(self, source: int = 0, edge_weight: float = 1.0):
        self.source = source
        self.edge_weight = edge_weight

    def _relax(self, superstep, values, incoming, has_msg, graph):
        """-> (new distances, mask of the vertices that improved)."""
        dev = values.device
        n_local = values.shape[0]
        if superstep == 0:
            new = torch.full_like(values, float("inf"))
            lo = graph.vertex_lo
            src_local = self.source - lo
            changed = torch.zeros(n_local, dtype=torch.bool, device=dev)
            if 0 <= src_local < n_local:
                new[src_local] = 0.0
                changed[src_local] = True
        else:
            cand = torch.where(has_msg.unsqueeze(1), incoming,
                               torch.full_like(incoming, float("inf")))
            new = torch.minimum(values, cand)
            changed = (new < values).any(dim=1)
        return new, changed

    def compute(self, superstep, values, incoming, has_msg, graph: LocalGraph):
        dev = values.device
        n_local = values.shape[0]
        new, changed = self._relax(superstep, values, incoming, has_msg,
                                   graph)
        edge_msgs = None
        if bool(changed.any()):
            counts = graph.row_ptr[1:] - graph.row_ptr[:-1]
            per_edge_changed = changed.repeat_interleave(counts)
            dist_per_edge = new.squeeze(1).repeat_interleave(counts)
            # each edge's own value (reference Vertex<V,E>) when the graph
            # carries them, else the constant
            w = (graph.edge_weight if graph.edge_weight is not None
                 else self.edge_weight)
            msgs = torch.where(per_edge_changed,
                               dist_per_edge + w,
                               torch.full_like(dist_per_edge, float("inf")))
            edge_msgs = msgs.unsqueeze(1)
        active = torch.zeros(n_local, dtype=torch.bool, device=dev)
        return new, edge_msgs, active

    def vertex_messages(self, superstep, values, incoming, has_msg,
                        graph: LocalGraph):
        """compute() with one message per vertex: an improved vertex sends
        its distance, and each edge adds its own weight on the way."""
        new, changed = self._relax(superstep, values, incoming, has_msg,
                                   graph)
        active = torch.zeros(values.shape[0], dtype=torch.bool,
                             device=values.device)
        return new, new.squeeze(1), changed, active


CC_MAX_VERTICES = 2 ** 24


class ConnectedComponentsComputation(Computation):
    """Label propagation with a min combiner: every vertex starts with its
    own global id as its label and sends it; afterwards a vertex adopts the
    smallest incoming label and, when that improved its own, sends it on.
    Vertices halt immediately; messages wake them. At the end label(v) is
    the smallest id with a path to v, which on a symmetrised edge list is
    the smallest id of v's weakly connected component.

    Labels are float32 vertex ids, exact up to 2^24; a larger graph raises
    ValueError here, before any table is built."""

    combiner = "min"
    msg_identity = float("inf")
    msg_dim = 1
    edge_op = "copy"

    def __init__(self, num_vertices: int):
        if num_vertices > CC_MAX_VERTICES:
            raise ValueError(
                f"connected components labels vertices with float32 ids, "
                f"which are exact only up to 2^24 = {CC_MAX_VERTICES} "
                f"vertices; got {num_vertices}")
        self.num_vertices = num_vertices

    def _relax(self, superstep, values, incoming, has_msg, graph):
        """-> (new labels, mask of the vertices that improved)."""
        n_local = values.shape[0]
        if superstep == 0:
            ids = torch.arange(graph.vertex_lo, graph.vertex_lo + n_local,
                               device=values.device)
            new = ids.to(values.dtype).unsqueeze(1)
            changed = torch.ones(n_local, dtype=torch.bool,
                                 device=values.device)
        else:
            cand = torch.where(has_msg.unsqueeze(1), incoming,
                               torch.full_like(incoming, float("inf")))
            new = torch.minimum(values, cand)
            changed = (new < values).any(dim=1)
        return new, changed

    def compute(self, superstep, values, incoming, has_msg, graph: LocalGraph):
        new, changed = self._relax(superstep, values, incoming, has_msg,
                                   graph)
        edge_msgs = None
        if bool(changed.any()):
            counts = graph.row_ptr[1:] - graph.row_ptr[:-1]
            label_per_edge = new.squeeze(1).repeat_interleave(counts)
            msgs = torch.where(changed.repeat_interleave(counts),
                               label_per_edge,
                               torch.full_like(label_per_edge, float("inf")))
            edge_msgs = msgs.unsqueeze(1)
        active = torch.zeros(values.shape[0], dtype=torch.bool,
                             device=values.device)
        return new, edge_msgs, active

    def vertex_messages(self, superstep, values, incoming, has_msg,
                        graph: LocalGraph):
        """compute() with one message per vertex: an improved vertex sends
        its label along all its out-edges as is."""
        new, changed = self._relax(superstep, values, incoming, has_msg,
                                   graph)
        active = torch.zeros(values.shape[0], dtype=torch.bool,
                             device=values.device)
        return new, new.squeeze(1), changed, active


def ring_plus_random_edges(num_vertices: int, out_degree: int, seed: int):
    """The whole edge list of make_ring_plus_random_graph on the CPU:
    (src int64 [n * deg], dst int64 [n * deg]), sources ascending."""
    g = make_ring_plus_random_graph(num_vertices, out_degree, 0, num_vertices,
                                    torch.device("cpu"), seed)
    src = torch.arange(num_vertices, dtype=torch.int64).repeat_interleave(
        out_degree)
    return src, g.edge_dst.to(torch.int64)


def symmetrise(src: torch.Tensor, dst: torch.Tensor):
    """Append every edge reversed: (src ++ dst, dst ++ src)."""
    return torch.cat([src, dst]), torch.cat([dst, src])


def make_ring_plus_random_graph(num_vertices: int, out_degree: int,
                                vertex_lo: int, vertex_hi: int,
                                device, seed: int) -> LocalGraph:
    """Synthetic graph: ring edge (connectivity) + random extra edges.

    Edges are a pure function of (seed, vertex id) via the counter RNG, so
    the GLOBAL graph is identical for every world size / partitioning — a
    2-rank run computes exactly the same PageRank as a 1-rank run."""
    from harmony_amd.ops.rng import rng_u32

    n_local = vertex_hi - vertex_lo
    deg = out_degree
    vs = torch.arange(vertex_lo, vertex_hi, dtype=torch.int64)
    ring = (vs + 1) % num_vertices                       # [n_local]
    if deg > 1:
        ctr = (vs.unsqueeze(1) * (deg - 1)
               + torch.arange(deg - 1, dtype=torch.int64))  # [n_local, deg-1]
        extra = rng_u32(seed & 0xFFFFFFFF, ctr.reshape(-1)) % num_vertices
        edge_dst = torch.cat([ring.unsqueeze(1),
                              extra.view(n_local, deg - 1)], dim=1).reshape(-1)
    else:
        edge_dst = ring
    row_ptr = torch.arange(0, (n_local + 1) * deg, deg, device=device)
    out_deg = torch.full((n_local,), float(deg), device=device)
    return LocalGraph(vertex_lo=vertex_lo, row_ptr=row_ptr,
                      edge_dst=edge_dst.to(device), out_degree=out_deg,
                      num_vertices_global=num_vertices)


def make_graph_from_edges(row_ptr: torch.Tensor, edge_dst: torch.Tensor,
                          edge_weight, vertex_lo: int, num_vertices: int,
                          device) -> LocalGraph:
    """LocalGraph over a loaded partition (dataloader.load_graph_partition):
    row_ptr/edge_dst are the local CSR of vertices [vertex_lo, vertex_lo +
    n_local); edge_weight is the per-edge value tensor or None."""
    row_ptr = row_ptr.to(device)
    out_deg = (row_ptr[1:] - row_ptr[:-1]).to(torch.float32)
    return LocalGraph(
        vertex_lo=vertex_lo, row_ptr=row_ptr, edge_dst=edge_dst.to(device),
        out_degree=out_deg, num_vertices_global=num_vertices,
        edge_weight=(None if edge_weight is None
                     else edge_weight.to(device, torch.float32)))
