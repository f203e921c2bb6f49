"""Distributed search over a torch.distributed process group: the torch-facing API of the two distributed
strategies, on one node.

Reference flow (main.c:110-197): root reads, Bcast x4, Scatter fixed-stride records, per-rank GPU work,
Gather x3, root prints. Here:
  * header (weights, |Seq1|, N, semantics) + Seq1: exact-count broadcasts through the process group
    (RCCL on GPU ranks, gloo on CPU ranks);
  * cost-balanced contiguous bounds (parallel/partition.py), valid for any world size;
  * partition "records", transport "shm": the root writes the CSR batch once into a node-shared /dev/shm
    window; every rank streams its own slice to its GPU (zero-copy, the wire formats of parallel/wire.py)
    and writes its results back in place — no payload collectives at all;
  * partition "offsets" (context parallel): every rank sees every record (the shm window,
    or one broadcast with transport "bcast") and searches its share of each record's offsets; the packed
    64-bit candidate keys are combined with ONE MAX all-reduce (the Reduce the reference never had) and the
    root decodes them.
Moving record payloads between ranks (several nodes, or device-resident batches over RCCL/xGMI) is the
native driver's job, one implementation: ./final --transport=rccl (csrc/src/device_batch.cpp).
"""
from __future__ import annotations

import os
import uuid
from typing import Optional

import numpy as np

from .. import _lib
from ..models.problem import Problem
from ..models.scoring import Semantics
from ..ops.align import (HipSearchEngine, decode_keys, device_count, keys_to_ordered_int64, ordered_int64_to_keys,
                        profile_offsets, search_cpu, search_hits_cpu, search_keys_cpu, search_report_cpu,
                        search_summary_cpu, search_targets_cpu, search_targets_summary_cpu, search_topk_cpu,
                         summary_bound, within_thresholds,
                         TargetSet, check_targets, _summary_args, _check_k, _check_radius, search_targets_hits_cpu,
                         search_targets_topk_cpu, search_targets_rank_cpu, _check_rank_m)
from ..utils.timer import PhaseTimer
from . import dist as D
from .partition import CPU_COST, GPU_COST, partition
from .wire import WireSlice


class NodeWindow:
    """A /dev/shm file mapped by every rank of the node: offsets[N+1] | results[N] | codes[T]."""

    def __init__(self, name: str, n: int, total: int, create: bool):
        self.path = f"/dev/shm/{name}"
        self.n, self.total = n, total
        self.off_bytes = 8 * (n + 1)
        self.res_bytes = (12 * n + 7) & ~7
        size = max(self.off_bytes + self.res_bytes + total, 8)
        mode = "w+" if create else "r+"
        self._mm = np.memmap(self.path, dtype=np.uint8, mode=mode, shape=(size,))
        self.offsets = self._mm[:self.off_bytes].view(np.int64)
        self.results = self._mm[self.off_bytes:self.off_bytes + 12 * n].view(_lib.RESULT_DTYPE)
        self.codes = self._mm[self.off_bytes + self.res_bytes:self.off_bytes + self.res_bytes + total]

    def close(self, unlink: bool):
        self._mm._mmap.close() if getattr(self._mm, "_mmap", None) is not None else None
        if unlink:
            try:
                os.unlink(self.path)
            except OSError:
                pass


class DistributedSearch:
    def __init__(self, ctx: D.DistContext, backend: str = "auto", transport: str = "auto", threads: int = 0,
                 device: Optional[int] = None, partition: str = "auto"):
        self.ctx = ctx
        if partition == "auto":  # record slices need the node-shared window; across nodes split offsets
            partition = "records" if (ctx.single_node and transport in ("auto", "shm")) else "offsets"
        if partition not in ("records", "offsets"):
            raise ValueError("partition must be auto|records|offsets")
        self.partition = partition
        if backend == "auto":
            backend = "hip" if device_count() > 0 else "cpu"
        self.backend = backend
        if transport == "auto":
            transport = "shm" if ctx.single_node else "bcast"
        if transport not in ("shm", "bcast"):
            raise ValueError("transport must be shm|bcast")
        if transport == "shm" and not ctx.single_node:
            raise ValueError("transport=shm needs every rank on one node")
        if partition == "records" and transport != "shm":
            raise ValueError("record slices move between ranks in ./final (--transport=rccl); the Python driver "
                             "runs them through a node-shared window (transport=shm, one node)")
        self.transport = transport
        self.threads = threads
        if backend == "hip" and device is None:
            device = ctx.local_rank % max(device_count(), 1)  # node-local rank -> GPU (ranks may share one)
        self.engine = HipSearchEngine(device) if backend == "hip" else None
        self.timer = PhaseTimer()
        if partition == "offsets" and ctx.distributed:
            # GPU ranks split tile lists, CPU ranks offset ranges: one engine kind for the whole group
            kinds = D.allreduce_max_int64(ctx, np.array([1 if self.engine else 0, 0 if self.engine else 1]))
            if kinds[0] and kinds[1]:
                raise ValueError("partition=offsets needs the same backend on every rank")

    def _compute(self, prob: Problem, sem: Semantics, codes, offsets, out):
        if self.engine is not None:
            # GPU ranks: the slice in the wire formats ./final's parser writes and bench.py streams
            # (parallel/wire.py), page-locked, searched zero-copy, decoded into the R12 result window
            ws = WireSlice.from_csr(codes, offsets)
            ws.alloc_results(self.engine)
            with _lib.Pinned(*ws.arrays()):
                ws.solve(self.engine)
            out.view(np.int32).reshape(-1, 3)[:] = ws.triples(self.engine)
        else:
            sub = Problem(prob.weights, prob.seq1, codes[offsets[0]:offsets[-1]], offsets - offsets[0])
            out[:] = search_cpu(sub, sem, self.threads)

    def _setup(self, problem: Optional[Problem], semantics):
        """Header + Seq1 broadcasts and the cost-balanced record bounds: (prob, sem, n, total, bounds)."""
        ctx = self.ctx
        sem = Semantics.parse(semantics)
        if ctx.is_root:
            hdr = np.array(problem.weights.as_list() + [problem.L1, problem.n, problem.total_chars, int(sem)],
                           np.int64)
        else:
            hdr = None
        hdr = D.bcast_array(ctx, hdr, 8, np.int64)
        w, L1, n, total, sem = list(hdr[:4]), int(hdr[4]), int(hdr[5]), int(hdr[6]), Semantics(int(hdr[7]))
        seq1 = D.bcast_array(ctx, problem.seq1 if ctx.is_root else None, L1, np.uint8)
        prob = Problem(w, seq1)
        if self.engine is not None:
            self.engine.set_problem(w, seq1, sem)
        bounds = partition(problem.lengths, L1, ctx.world, GPU_COST if self.backend == "hip" else CPU_COST) \
            if ctx.is_root else None
        bounds = D.bcast_array(ctx, bounds, ctx.world + 1, np.int64)
        return prob, sem, n, total, bounds

    def run(self, problem: Optional[Problem], semantics=Semantics.REFERENCE) -> Optional[np.ndarray]:
        ctx, T = self.ctx, self.timer
        with T.phase("bcast"):
            prob, sem, n, total, bounds = self._setup(problem, semantics)
        b, e = int(bounds[ctx.rank]), int(bounds[ctx.rank + 1])
        if self.partition == "offsets":
            return self._run_offsets(problem, prob, sem, n, total)
        return self._run_shm(problem, prob, sem, n, total, b, e)

    def _open_window(self, problem, n, total) -> NodeWindow:
        """The node-shared input window: the root writes the batch once, every rank maps it."""
        ctx = self.ctx
        name_arr = None
        if ctx.is_root:  # fixed 20-byte name: "moc_win_" + 12 hex digits
            name_arr = np.frombuffer(f"moc_win_{uuid.uuid4().hex[:12]}".encode(), np.uint8)
        name = bytes(D.bcast_array(ctx, name_arr, 20, np.uint8)).decode()
        win = None
        if ctx.is_root:
            win = NodeWindow(name, n, total, create=True)
            win.offsets[:] = problem.offsets
            win.codes[:] = problem.codes
            win._mm.flush()
        D.barrier(ctx)
        if not ctx.is_root:
            win = NodeWindow(name, n, total, create=False)
        return win

    def run_topk(self, problem: Optional[Problem], K: int, semantics=Semantics.REFERENCE,
                 radius: int = 0) -> Optional[np.ndarray]:
        """The K best offsets of every record (ops.align.search_topk_cpu's int32 [n, K, 3] rows) for the
        ``records`` partition: every rank searches its cost-balanced slice of the node-shared input window, and
        the root collects the rows with one MAX all-reduce of an array each rank fills only in its own slice
        (no new transport). One node; byte letters through the engines' top-K calls. ``radius`` > 0 (the same on
        every rank): the K best distinct placements (ops.align.search_topk_cpu)."""
        if self.partition != "records":
            raise ValueError("top-K runs on record slices (--partition records, one node): the offsets partition "
                             "combines one packed key per record and cannot carry K rows")
        ctx, T = self.ctx, self.timer
        with T.phase("bcast"):
            prob, sem, n, total, bounds = self._setup(problem, semantics)
        b, e = int(bounds[ctx.rank]), int(bounds[ctx.rank + 1])
        with T.phase("distribute"):
            win = self._open_window(problem, n, total)
        with T.phase("compute"):
            rows = np.full((n, K, 3), np.iinfo(np.int64).min, np.int64)
            if e > b:
                offsets = np.asarray(win.offsets[b:e + 1])
                if self.engine is not None:
                    rows[b:e] = self.engine.solve_topk(np.asarray(win.codes), offsets, K, radius)
                else:
                    sub = Problem(prob.weights, prob.seq1, np.asarray(win.codes[offsets[0]:offsets[-1]]),
                                  offsets - offsets[0])
                    rows[b:e] = search_topk_cpu(sub, K, sem, self.threads, radius)
        with T.phase("gather"):
            rows = D.allreduce_max_int64(ctx, rows.reshape(-1)).reshape(n, K, 3)
            D.barrier(ctx)
            win.close(unlink=ctx.is_root)
        return rows.astype(np.int32) if ctx.is_root else None

    def run_hits(self, problem: Optional[Problem], min_score=None, within=None, semantics=Semantics.REFERENCE,
                 radius: int = 0):
        """Threshold hits (ops.align.search_hits_cpu's ``(rows, hoffsets)``; exactly one of ``min_score`` and
        ``within``, the same on every rank) together with the search's own rows, for the ``records`` partition:
        every rank computes its cost-balanced slice of the node-shared input window; the root collects the counts and then the rows, each
        with one MAX all-reduce of an int64 array that a rank fills only in its own slice, INT64_MIN elsewhere (no
        new transport). Returns ``(results, rows, hoffsets)`` on the root, else None. One node; byte letters
        through the engines' hits calls. ``radius`` > 0 (the same on every rank): the distinct placements among the
        hits (ops.align.search_hits_cpu)."""
        if self.partition != "records":
            raise ValueError("hits run on record slices (--partition records, one node): the offsets partition "
                             "combines one packed key per record and cannot carry a list of rows")
        if (min_score is None) == (within is None):
            raise ValueError("hits: give exactly one of min_score, within")
        if within is not None and int(within) < 0:
            raise ValueError(f"hits: within must be >= 0, got {int(within)}")
        ctx, T = self.ctx, self.timer
        with T.phase("bcast"):
            prob, sem, n, total, bounds = self._setup(problem, semantics)
        b, e = int(bounds[ctx.rank]), int(bounds[ctx.rank + 1])
        with T.phase("distribute"):
            win = self._open_window(problem, n, total)
        lo = np.iinfo(np.int64).min

        def kw(scores):  # the slice's thresholds from the search just done: no second search for `within`
            return {"min_score": int(min_score)} if min_score is not None else \
                {"thresholds": within_thresholds(scores, within)}

        with T.phase("compute"):
            best = np.full((n, 3), lo, np.int64)
            counts = np.full(n, lo, np.int64)
            mine = np.zeros((0, 3), np.int32)
            if e > b:
                offsets = np.asarray(win.offsets[b:e + 1])
                if self.engine is not None:
                    codes = np.asarray(win.codes)
                    best[b:e] = self.engine.solve(codes, offsets).view(np.int32).reshape(-1, 3)
                    mine, h = self.engine.solve_hits(codes, offsets, radius=radius, **kw(best[b:e, 0]))
                else:
                    sub = Problem(prob.weights, prob.seq1, np.asarray(win.codes[offsets[0]:offsets[-1]]),
                                  offsets - offsets[0])
                    best[b:e] = search_cpu(sub, sem, self.threads).view(np.int32).reshape(-1, 3)
                    mine, h = search_hits_cpu(sub, semantics=sem, threads=self.threads, radius=radius, **kw(best[b:e, 0]))
                counts[b:e] = np.diff(h)
        with T.phase("gather"):
            counts = D.allreduce_max_int64(ctx, counts)
            best = D.allreduce_max_int64(ctx, best.reshape(-1)).reshape(n, 3)
            hoffsets = np.zeros(n + 1, np.int64)
            np.cumsum(counts, out=hoffsets[1:])
            rows = np.full((int(hoffsets[-1]), 3), lo, np.int64)
            rows[hoffsets[b]:hoffsets[e]] = mine
            rows = D.allreduce_max_int64(ctx, rows.reshape(-1)).reshape(-1, 3)
            D.barrier(ctx)
            win.close(unlink=ctx.is_root)
        return (best.astype(np.int32), rows.astype(np.int32), hoffsets) if ctx.is_root else None

    def run_summary(self, problem: Optional[Problem], bins: int = 0, lo: int = 0, width: int = 1,
                    semantics=Semantics.REFERENCE):
        """The profile summary (ops.align.search_summary_cpu's ``(summary, hist)``; the same ``bins``, ``lo`` and
        ``width`` on every rank) for the ``records`` partition: every rank summarises its cost-balanced slice of the
        node-shared input window into int64 arrays that are INT64_MIN outside the slice — the histogram widened to
        int64 for the trip — and one MAX all-reduce of each combines them (no new transport). ``summary[:, 4:7]`` are
        the search's rows. Returns ``(summary, hist)`` on the root (``hist`` None with ``bins = 0``), else None. The
        exactness bound is checked for the whole batch on the root and every rank raises the same ValueError. One
        node; byte letters through the engines' summary calls."""
        if self.partition != "records":
            raise ValueError("the summary runs on record slices (--partition records, one node): the offsets "
                             "partition combines one packed key per record and cannot carry a record's moments")
        bins, lo, width = _summary_args(bins, lo, width)
        ctx, T = self.ctx, self.timer
        sem = Semantics.parse(semantics)
        bad = None
        if ctx.is_root:  # a slice inside the bound where the batch is not would leave the ranks in different states
            L2 = np.asarray(problem.lengths, dtype=np.int64)
            cmax = int(np.diff(profile_offsets(problem.L1, L2, sem)).max()) if problem.n else 0
            w = max(abs(int(x)) for x in problem.weights.as_list())
            limit = summary_bound(w, int(L2.max()) if problem.n else 0)
            bad = np.array([cmax if cmax > limit else 0, limit], np.int64)
        bad = D.bcast_array(ctx, bad, 2, np.int64)
        if int(bad[0]):
            raise ValueError(f"summary: exactness bound: a profile of {int(bad[0])} entries may overflow the int64 sum "
                             f"of squares (at most {int(bad[1])} entries per record are exact for this batch)")
        with T.phase("bcast"):
            prob, sem, n, total, bounds = self._setup(problem, sem)
        b, e = int(bounds[ctx.rank]), int(bounds[ctx.rank + 1])
        with T.phase("distribute"):
            win = self._open_window(problem, n, total)
        none = np.iinfo(np.int64).min
        with T.phase("compute"):
            summary = np.full((n, 7), none, np.int64)
            hist = np.full((n, bins), none, np.int64)
            if e > b:
                offsets = np.asarray(win.offsets[b:e + 1])
                if self.engine is not None:
                    s, h = self.engine.solve_summary(np.asarray(win.codes), offsets, bins, lo, width)
                else:
                    sub = Problem(prob.weights, prob.seq1, np.asarray(win.codes[offsets[0]:offsets[-1]]),
                                  offsets - offsets[0])
                    s, h = search_summary_cpu(sub, bins, lo, width, sem, self.threads)
                summary[b:e] = s
                if bins:
                    hist[b:e] = h
        with T.phase("gather"):
            summary = D.allreduce_max_int64(ctx, summary.reshape(-1)).reshape(n, 7)
            if bins:
                hist = D.allreduce_max_int64(ctx, hist.reshape(-1)).reshape(n, bins)
            D.barrier(ctx)
            win.close(unlink=ctx.is_root)
        return (summary, hist.astype(np.int32) if bins else None) if ctx.is_root else None

    def run_targets(self, problem: Optional[Problem], targets=None, semantics=Semantics.REFERENCE):
        """Multi-target search (ops.align.search_targets_cpu's int32 [n, T, 3] rows; ``problem.seq1`` is the catalog
        of ``targets``, a TargetSet or its starts, both needed on the root only) for the ``records`` partition: the
        root broadcasts the starts, every rank searches its cost-balanced slice of the node-shared input window
        against every target, and one MAX all-reduce of an int64 array that a rank fills only in its own slice
        collects the rows (no new transport). Returns the rows on the root, else None. An invalid target set raises
        the same ValueError on every rank. One node; byte letters through the engines' targets calls."""
        if self.partition != "records":
            raise ValueError("the multi-target search runs on record slices (--partition records, one node): the "
                             "offsets partition combines one packed key per record and cannot carry T rows")
        ctx, T = self.ctx, self.timer
        sem = Semantics.parse(semantics)
        hdr = None
        if ctx.is_root:
            starts = np.ascontiguousarray(targets.starts if isinstance(targets, TargetSet) else targets,
                                          dtype=np.int64).reshape(-1)
            hdr = np.array([starts.shape[0], problem.L1], np.int64)
        hdr = D.bcast_array(ctx, hdr, 2, np.int64)
        starts = D.bcast_array(ctx, starts if ctx.is_root else None, int(hdr[0]), np.int64)
        starts = check_targets(starts, int(hdr[1]))  # every rank raises alike
        nt = starts.shape[0] - 1
        with T.phase("bcast"):
            prob, sem, n, total, bounds = self._setup(problem, sem)
        b, e = int(bounds[ctx.rank]), int(bounds[ctx.rank + 1])
        with T.phase("distribute"):
            win = self._open_window(problem, n, total)
        with T.phase("compute"):
            rows = np.full((n, nt, 3), np.iinfo(np.int64).min, np.int64)
            if e > b:
                offsets = np.asarray(win.offsets[b:e + 1])
                if self.engine is not None:
                    rows[b:e] = self.engine.solve_targets(np.asarray(win.codes), offsets, starts)
                else:
                    sub = Problem(prob.weights, prob.seq1, np.asarray(win.codes[offsets[0]:offsets[-1]]),
                                  offsets - offsets[0])
                    rows[b:e] = search_targets_cpu(sub, starts, sem, self.threads)
        with T.phase("gather"):
            rows = D.allreduce_max_int64(ctx, rows.reshape(-1)).reshape(n, nt, 3)
            D.barrier(ctx)
            win.close(unlink=ctx.is_root)
        return rows.astype(np.int32) if ctx.is_root else None

    def _bcast_starts(self, problem: Optional[Problem], targets) -> np.ndarray:
        """The root's target set (a TargetSet or its starts) as checked starts on every rank; an invalid set raises
        the same ValueError on every rank."""
        ctx = self.ctx
        hdr = None
        starts = None
        if ctx.is_root:
            starts = np.ascontiguousarray(targets.starts if isinstance(targets, TargetSet) else targets,
                                          dtype=np.int64).reshape(-1)
            hdr = np.array([starts.shape[0], problem.L1], np.int64)
        hdr = D.bcast_array(ctx, hdr, 2, np.int64)
        starts = D.bcast_array(ctx, starts if ctx.is_root else None, int(hdr[0]), np.int64)
        return check_targets(starts, int(hdr[1]))

    def run_targets_topk(self, problem: Optional[Problem], targets=None, K: int = 1, semantics=Semantics.REFERENCE,
                         radius: int = 0):
        """Per-target top-K (ops.align.search_targets_topk_cpu's int32 [n, T, K, 3] rows; ``K`` the same on every rank,
        ``targets`` as :meth:`run_targets`) for the ``records`` partition: every rank ranks its cost-balanced slice of
        the node-shared input window against every target, and one MAX all-reduce of an int64 array that is INT64_MIN
        outside the rank's slice collects the rows (no new transport). Returns the rows on the root, else None. One
        node; byte letters through the engines' per-target top-K calls. ``radius`` > 0 (the same on every rank): the
        distinct placements per target, search_targets_topk_cpu's."""
        if self.partition != "records":
            raise ValueError("per-target top-K runs on record slices (--partition records, one node): the offsets "
                             "partition combines one packed key per record and cannot carry T K rows")
        ctx, T = self.ctx, self.timer
        sem = Semantics.parse(semantics)
        starts = self._bcast_starts(problem, targets)  # the target set's errors come first
        K = _check_k(K)
        radius = _check_radius(radius)
        nt = starts.shape[0] - 1
        with T.phase("bcast"):
            prob, sem, n, total, bounds = self._setup(problem, sem)
        b, e = int(bounds[ctx.rank]), int(bounds[ctx.rank + 1])
        with T.phase("distribute"):
            win = self._open_window(problem, n, total)
        with T.phase("compute"):
            rows = np.full((n, nt, K, 3), np.iinfo(np.int64).min, np.int64)
            if e > b:
                offsets = np.asarray(win.offsets[b:e + 1])
                if self.engine is not None:
                    rows[b:e] = self.engine.solve_targets_topk(np.asarray(win.codes), offsets, starts, K, radius)
                else:
                    sub = Problem(prob.weights, prob.seq1, np.asarray(win.codes[offsets[0]:offsets[-1]]),
                                  offsets - offsets[0])
                    rows[b:e] = search_targets_topk_cpu(sub, starts, K, sem, self.threads, radius)
        with T.phase("gather"):
            rows = D.allreduce_max_int64(ctx, rows.reshape(-1)).reshape(n, nt, K, 3)
            D.barrier(ctx)
            win.close(unlink=ctx.is_root)
        return rows.astype(np.int32) if ctx.is_root else None

    def run_targets_rank(self, problem: Optional[Problem], targets=None, M: int = 1, semantics=Semantics.REFERENCE):
        """Target ranking (ops.align.search_targets_rank_cpu's int32 [n, M, 4] rows; ``M`` the same on every rank,
        ``targets`` as :meth:`run_targets`) for the ``records`` partition: every rank ranks the targets of its
        cost-balanced slice of the node-shared input window, and one MAX all-reduce of an int64 array that is
        INT64_MIN outside the rank's slice collects the n M rows (no new transport; the n T pair rows exist nowhere).
        Returns the rows on the root, else None. One node; byte letters through the engines' rank calls."""
        if self.partition != "records":
            raise ValueError("the target ranking runs on record slices (--partition records, one node): the offsets "
                             "partition combines one packed key per record and cannot carry M rows")
        ctx, T = self.ctx, self.timer
        sem = Semantics.parse(semantics)
        starts = self._bcast_starts(problem, targets)  # the target set's errors come first
        M = _check_rank_m(M)
        with T.phase("bcast"):
            prob, sem, n, total, bounds = self._setup(problem, sem)
        b, e = int(bounds[ctx.rank]), int(bounds[ctx.rank + 1])
        with T.phase("distribute"):
            win = self._open_window(problem, n, total)
        with T.phase("compute"):
            rows = np.full((n, M, 4), np.iinfo(np.int64).min, np.int64)
            if e > b:
                offsets = np.asarray(win.offsets[b:e + 1])
                if self.engine is not None:
                    rows[b:e] = self.engine.solve_targets_rank(np.asarray(win.codes), offsets, starts, M)
                else:
                    sub = Problem(prob.weights, prob.seq1, np.asarray(win.codes[offsets[0]:offsets[-1]]),
                                  offsets - offsets[0])
                    rows[b:e] = search_targets_rank_cpu(sub, starts, M, sem, self.threads)
        with T.phase("gather"):
            rows = D.allreduce_max_int64(ctx, rows.reshape(-1)).reshape(n, M, 4)
            D.barrier(ctx)
            win.close(unlink=ctx.is_root)
        return rows.astype(np.int32) if ctx.is_root else None

    def run_targets_hits(self, problem: Optional[Problem], targets=None, min_score=None, within=None,
                         semantics=Semantics.REFERENCE, radius: int = 0):
        """Per-target threshold hits (ops.align.search_targets_hits_cpu's ``(rows, toffsets)``; exactly one of
        ``min_score`` and ``within``, the same on every rank; ``targets`` as :meth:`run_targets`) together with the
        multi-target rows, for the ``records`` partition: every rank computes its cost-balanced slice of the
        node-shared input window; the root collects the pairs' counts and then the rows as :meth:`run_hits` does, each
        with one MAX all-reduce of an int64 array that is INT64_MIN outside the rank's slice. ``within`` takes each
        pair's own best score from the multi-target search of the same slice. Returns ``(best, rows, toffsets)`` on
        the root — ``best`` the int32 [n, T, 3] multi-target rows — else None. One node; byte letters through the
        engines' per-target hits calls. ``radius`` > 0 (the same on every rank): the distinct placements per target,
        search_targets_hits_cpu's."""
        if self.partition != "records":
            raise ValueError("per-target hits run on record slices (--partition records, one node): the offsets "
                             "partition combines one packed key per record and cannot carry a list of rows")
        ctx, T = self.ctx, self.timer
        sem = Semantics.parse(semantics)
        starts = self._bcast_starts(problem, targets)  # the target set's errors come first
        if (min_score is None) == (within is None):
            raise ValueError("hits: give exactly one of min_score, within")
        if within is not None and int(within) < 0:
            raise ValueError(f"hits: within must be >= 0, got {int(within)}")
        radius = _check_radius(radius)
        nt = starts.shape[0] - 1
        with T.phase("bcast"):
            prob, sem, n, total, bounds = self._setup(problem, sem)
        b, e = int(bounds[ctx.rank]), int(bounds[ctx.rank + 1])
        with T.phase("distribute"):
            win = self._open_window(problem, n, total)
        lo = np.iinfo(np.int64).min

        def kw(scores):  # the slice's thresholds from the multi-target search just done
            return {"min_score": int(min_score)} if min_score is not None else \
                {"thresholds": within_thresholds(scores, within).reshape(-1, nt)}

        with T.phase("compute"):
            best = np.full((n, nt, 3), lo, np.int64)
            counts = np.full(n * nt, lo, np.int64)
            mine = np.zeros((0, 3), np.int32)
            if e > b:
                offsets = np.asarray(win.offsets[b:e + 1])
                if self.engine is not None:
                    codes = np.asarray(win.codes)
                    best[b:e] = self.engine.solve_targets(codes, offsets, starts)
                    mine, h = self.engine.solve_targets_hits(codes, offsets, starts, radius=radius, **kw(best[b:e, :, 0]))
                else:
                    sub = Problem(prob.weights, prob.seq1, np.asarray(win.codes[offsets[0]:offsets[-1]]),
                                  offsets - offsets[0])
                    best[b:e] = search_targets_cpu(sub, starts, sem, self.threads)
                    mine, h = search_targets_hits_cpu(sub, starts, semantics=sem, threads=self.threads, radius=radius,
                                                      **kw(best[b:e, :, 0]))
                counts[b * nt:e * nt] = np.diff(h)
        with T.phase("gather"):
            counts = D.allreduce_max_int64(ctx, counts)
            best = D.allreduce_max_int64(ctx, best.reshape(-1)).reshape(n, nt, 3)
            toffsets = np.zeros(n * nt + 1, np.int64)
            np.cumsum(counts, out=toffsets[1:])
            rows = np.full((int(toffsets[-1]), 3), lo, np.int64)
            rows[toffsets[b * nt]:toffsets[e * nt]] = mine
            rows = D.allreduce_max_int64(ctx, rows.reshape(-1)).reshape(-1, 3)
            D.barrier(ctx)
            win.close(unlink=ctx.is_root)
        return (best.astype(np.int32), rows.astype(np.int32), toffsets) if ctx.is_root else None

    def run_targets_summary(self, problem: Optional[Problem], targets=None, bins: int = 0, lo: int = 0, width: int = 1,
                            semantics=Semantics.REFERENCE):
        """The per-target profile summary (ops.align.search_targets_summary_cpu's ``(summary, hist)``, int64
        [n, T, 7] and int32 [n, T, bins]; ``problem.seq1`` is the catalog of ``targets``, both needed on the root
        only; the same ``bins``, ``lo`` and ``width`` on every rank) for the ``records`` partition: as
        :meth:`run_targets` the root broadcasts the starts, and as :meth:`run_summary` every rank fills int64 arrays
        that are INT64_MIN outside its slice and one MAX all-reduce of each combines them (no new transport).
        Returns ``(summary, hist)`` on the root (``hist`` None with ``bins = 0``), else None. The target set and the
        exactness bound of the whole batch are checked on the root, and every rank raises the same ValueError. One
        node; byte letters through the engines' per-target summary calls."""
        if self.partition != "records":
            raise ValueError("the per-target summary runs on record slices (--partition records, one node): the "
                             "offsets partition combines one packed key per record and cannot carry T summary rows")
        bins, lo, width = _summary_args(bins, lo, width)
        ctx, T = self.ctx, self.timer
        sem = Semantics.parse(semantics)
        hdr = None
        if ctx.is_root:
            starts = np.ascontiguousarray(targets.starts if isinstance(targets, TargetSet) else targets,
                                          dtype=np.int64).reshape(-1)
            hdr = np.array([starts.shape[0], problem.L1], np.int64)
        hdr = D.bcast_array(ctx, hdr, 2, np.int64)
        starts = D.bcast_array(ctx, starts if ctx.is_root else None, int(hdr[0]), np.int64)
        starts = check_targets(starts, int(hdr[1]))  # every rank raises alike
        nt = starts.shape[0] - 1
        bad = None
        if ctx.is_root:  # the largest target profile of the whole batch: the longest target, the shortest record in it
            L2 = np.asarray(problem.lengths, dtype=np.int64)
            longest = int(np.diff(starts).max())
            fits = L2[(L2 >= 1) & (L2 <= longest)]
            cmax = 0
            if fits.size:
                shortest = int(fits.min())
                cmax = longest - shortest + (1 if sem == Semantics.SPEC or shortest == longest else 0)
            w = max(abs(int(x)) for x in problem.weights.as_list())
            limit = summary_bound(w, int(L2.max()) if problem.n else 0)
            bad = np.array([cmax if cmax > limit else 0, limit], np.int64)
        bad = D.bcast_array(ctx, bad, 2, np.int64)
        if int(bad[0]):
            raise ValueError(f"summary: exactness bound: a target profile of {int(bad[0])} entries may overflow the "
                             f"int64 sum of squares (at most {int(bad[1])} entries per pair are exact for this batch)")
        with T.phase("bcast"):
            prob, sem, n, total, bounds = self._setup(problem, sem)
        b, e = int(bounds[ctx.rank]), int(bounds[ctx.rank + 1])
        with T.phase("distribute"):
            win = self._open_window(problem, n, total)
        none = np.iinfo(np.int64).min
        with T.phase("compute"):
            summary = np.full((n, nt, 7), none, np.int64)
            hist = np.full((n, nt, bins), none, np.int64)
            if e > b:
                offsets = np.asarray(win.offsets[b:e + 1])
                if self.engine is not None:
                    s, h = self.engine.solve_targets_summary(np.asarray(win.codes), offsets, starts, bins, lo, width)
                else:
                    sub = Problem(prob.weights, prob.seq1, np.asarray(win.codes[offsets[0]:offsets[-1]]),
                                  offsets - offsets[0])
                    s, h = search_targets_summary_cpu(sub, starts, bins, lo, width, sem, self.threads)
                summary[b:e] = s
                if bins:
                    hist[b:e] = h
        with T.phase("gather"):
            summary = D.allreduce_max_int64(ctx, summary.reshape(-1)).reshape(n, nt, 7)
            if bins:
                hist = D.allreduce_max_int64(ctx, hist.reshape(-1)).reshape(n, nt, bins)
            D.barrier(ctx)
            win.close(unlink=ctx.is_root)
        return (summary, hist.astype(np.int32) if bins else None) if ctx.is_root else None

    def report(self, problem: Problem, rows: np.ndarray):
        """Root only: ``(counts, marks)`` of the search's rows (ops.align.search_report_cpu's outputs, with the
        marker bytes), on this rank's engine — the GPU's report kernels or the CPU engine. The report is one pass
        over the letters, so the ranks do not share it."""
        if self.engine is not None:  # the search's _setup left this problem in the engine
            return self.engine.report(problem.codes, problem.offsets, rows, marks=True)
        return search_report_cpu(problem, rows, marks=True, threads=self.threads)

    def _run_shm(self, problem, prob, sem, n, total, b, e):
        ctx, T = self.ctx, self.timer
        with T.phase("distribute"):
            name_arr = None
            if ctx.is_root:  # fixed 20-byte name: "moc_win_" + 12 hex digits
                name_arr = np.frombuffer(f"moc_win_{uuid.uuid4().hex[:12]}".encode(), np.uint8)
            name = bytes(D.bcast_array(ctx, name_arr, 20, np.uint8)).decode()
            win = None
            if ctx.is_root:
                win = NodeWindow(name, n, total, create=True)
                win.offsets[:] = problem.offsets
                win.codes[:] = problem.codes
                win._mm.flush()
            D.barrier(ctx)
            if not ctx.is_root:
                win = NodeWindow(name, n, total, create=False)
        with T.phase("compute"):
            if e > b:
                self._compute(prob, sem, win.codes, win.offsets[b:e + 1], win.results[b:e])
        with T.phase("gather"):
            D.barrier(ctx)
            out = np.array(win.results) if ctx.is_root else None
            D.barrier(ctx)
            win.close(unlink=ctx.is_root)
        return out

    def _keys(self, prob: Problem, sem: Semantics, codes, offsets) -> np.ndarray:
        if self.engine is not None:
            return self.engine.search_keys(codes, offsets, self.ctx.rank, self.ctx.world)
        sub = Problem(prob.weights, prob.seq1, codes[offsets[0]:offsets[-1]], offsets - offsets[0])
        return search_keys_cpu(sub, self.ctx.rank, self.ctx.world, sem, self.threads)

    def _run_offsets(self, problem, prob, sem, n, total):
        ctx, T = self.ctx, self.timer
        with T.phase("distribute"):  # every rank needs every record
            if self.transport == "shm":
                name_arr = None
                if ctx.is_root:
                    name_arr = np.frombuffer(f"moc_win_{uuid.uuid4().hex[:12]}".encode(), np.uint8)
                name = bytes(D.bcast_array(ctx, name_arr, 20, np.uint8)).decode()
                win = None
                if ctx.is_root:
                    win = NodeWindow(name, n, total, create=True)
                    win.offsets[:] = problem.offsets
                    win.codes[:] = problem.codes
                    win._mm.flush()
                D.barrier(ctx)
                if not ctx.is_root:
                    win = NodeWindow(name, n, total, create=False)
                codes, offsets = win.codes, win.offsets
            else:
                win = None
                offsets = D.bcast_array(ctx, problem.offsets if ctx.is_root else None, n + 1, np.int64)
                codes = D.bcast_array(ctx, problem.codes if ctx.is_root else None, total, np.uint8)
        with T.phase("compute"):
            keys = self._keys(prob, sem, np.asarray(codes), np.asarray(offsets)) if n else np.zeros(0, np.uint64)
        with T.phase("gather"):
            best = ordered_int64_to_keys(D.allreduce_max_int64(ctx, keys_to_ordered_int64(keys)))
            out = decode_keys(best, Problem(prob.weights, prob.seq1, np.asarray(codes), np.asarray(offsets))) \
                if ctx.is_root else None
            if win is not None:
                D.barrier(ctx)
                win.close(unlink=ctx.is_root)
        return out
