"""How a unit's recorded plans are driven under data parallelism: the captured graph with its heartbeat, the fall-back the ranks
agree on, and the host loop with merged enqueues.  A base class of `engine.UnitEngine`; it never touches a kernel helper."""
import logging
import os
import time

import torch


class DpStallError(RuntimeError):
    """The captured data-parallel loop stopped making progress (`UnitEngine._hb_wait`): a collective inside the graph hangs."""


class DpLoop:
    """The data-parallel run loop of `UnitEngine` (plan A -> all-reduce -> plan B, see `_run_dp`).

    Reads of the engine: `plan_a`, `plan_a2`, `plan_b` (the recorded plans), `bucket` (dp.GradBucket), `use_graph`, `world`, `group`, `dev`.
    Owns: `dp_path`, `dp_fallbacks`, `_dp_graph`, `_dp_graph_failed` and the heartbeat `_hb_dev`, `_hb_host`, `_hb_issued`.  The engine
    drops `_dp_graph` when it records its plans anew (`_recover`)."""

    # backends whose collectives can be captured into a graph (torch's "nccl" = RCCL on ROCm); a test adds "gloo" to exercise the agreement
    DP_GRAPH_BACKENDS = ("nccl",)
    DP_HB_BATCH = 32                                                   # captured replays between two looks at the heartbeat
    DP_STALL_S = float(os.environ.get("RDO_DP_STALL_S", 120))          # no heartbeat for this long = the captured loop hangs

    def _dp_init(self):
        self.dp_path = None                    # "graph" | "host" once a data-parallel run has started (_run_dp)
        self._dp_graph, self._dp_graph_failed = None, False
        self.dp_fallbacks = 0                  # captures the ranks agreed to drop (this unit then runs the host loop on every rank)
        self._hb_dev = self._hb_host = None    # heartbeat of the captured loop (`_dp_capture`)
        self._hb_issued = 0

    def _dp_iteration(self, graph, first=True, last=True):
        """One data-parallel iteration on the current stream: plan A -> all-reduce of the front of the bucket (asynchronous, on the
        process group's stream) overlapped with plan A2 = the last weight gradient -> all-reduce of the rest -> plan B.
        Inside a host-driven run of several iterations plan B of iteration i and plan A of iteration i + 1 go out as ONE graph launch
        (`first=False`: plan A was enqueued with the previous iteration's plan B; `last=False`: enqueue the next plan A with this
        plan B): two host enqueues per iteration and collective instead of three -- the small units are host-bound in this loop."""
        if first:
            self.plan_a.run(1, graph=graph)
        self.bucket.reduce(between=None if self.plan_a2 is None else (lambda: self.plan_a2.run(1, graph=graph)))
        if last:
            self.plan_b.run(1, graph=graph)
        else:
            self.plan_b.run_then(self.plan_a, graph=graph)

    def _dp_capture(self):
        """One data-parallel iteration -- the recorded kernels of the plans AND the collectives -- as one graph, closed by the heartbeat:
        a device counter incremented and copied to pinned host memory by the graph's last two nodes.  torch's NCCL watchdog does not see
        collectives replayed from a graph; the heartbeat is what tells the host that replays still complete (`_hb_wait`).
        The capture is thread-local, like the plans' own (csrc/runtime.hip): a process group brings threads of its own -- torch's
        watchdog polls the events of the eager iteration's collectives every 100 ms or so -- and under torch's default ("global") an
        event query by ANY thread while this one captures invalidates the capture and fails in the thread that made it; there it is
        nobody's exception to catch, and the process aborts."""
        if self._hb_dev is None:
            self._hb_dev = torch.zeros(1, dtype=torch.int64, device=self.dev)
            self._hb_host = torch.zeros(1, dtype=torch.int64).pin_memory()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            self._dp_iteration(False)
            self._hb_dev.add_(1)
            self._hb_host.copy_(self._hb_dev, non_blocking=True)
        return g

    def _hb_wait(self, target):
        """Block until `target` captured replays have completed (heartbeat in pinned memory: no device synchronisation, which would hang
        with the loop).  No progress for DP_STALL_S seconds -> `DpStallError`: the process cannot recover a hung collective; the
        application decides (bench.py exits with status 86 and its launcher / supervisor starts FRESH children on the host loop)."""
        if self._hb_host is None or target <= 0:
            return
        seen, t_last = int(self._hb_host[0]), time.monotonic()
        while seen < target:
            time.sleep(0.0005)
            now = int(self._hb_host[0])
            if now != seen:
                seen, t_last = now, time.monotonic()
            elif time.monotonic() - t_last > self.DP_STALL_S:
                raise DpStallError(f"rank {self._rank()}: the captured data-parallel loop made no progress for {self.DP_STALL_S:.0f} s "
                                   f"({seen} of {self._hb_issued} replays completed) -- a collective inside the graph hangs")

    def dp_drain(self):
        """Wait (heartbeat, with the stall deadline) for every captured replay issued so far: call it before anything that synchronises
        the device behind a data-parallel run -- a plain synchronisation behind a hung graph would never return."""
        if self._dp_graph is not None:
            self._hb_wait(self._hb_issued)

    def _run_dp(self, n):
        """n data-parallel iterations.  With the RCCL backend (round 5: the DEFAULT; `RDO_DP_GRAPH=0` keeps the host loop) the whole
        iteration -- the recorded kernels of the three plans AND the collectives -- is captured once per unit into ONE graph
        (torch.cuda.graph) and replayed with no host work in between: the host-driven loop (plan A -> all-reduce -> plan B, each plan
        a graph replay, the collective enqueued by torch.distributed in between) costs two to three enqueues per unit-iteration, which
        the sixteen <= 50-us units cannot hide (+13 % on one rank against +5 % captured, `extra.dp_overhead_one_rank` of the bench
        line re-measures both on every run).  The ranks AGREE on the outcome of the capture (MIN all-reduce of an "ok" flag) before
        anyone replays: a rank never replays a graph with collectives while another runs the host loop; a unit whose capture fails
        on any rank runs the host loop on every rank (`dp_fallbacks` counts them).  The eager iteration in front of the capture is
        OUTSIDE the try: it is an ordinary iteration on every rank whatever the capture does afterwards, so all ranks run the same
        number of iterations (an exception in it is a real failure and propagates).  Replays are watched through a heartbeat
        (`_dp_capture`, `_hb_wait`).  Other backends (gloo in the CPU / one-GPU tests): host loop.  `self.dp_path` says which loop
        ran ("graph" / "host"); every rank logs it, the bench line carries it per unit."""
        dist = torch.distributed
        comm = self.world > 1 or (dist.is_available() and dist.is_initialized())
        want = (self.use_graph and os.environ.get("RDO_DP_GRAPH", "1") == "1" and comm
                and dist.get_backend(self.group) in self.DP_GRAPH_BACKENDS)
        if want and self._dp_graph is None and not self._dp_graph_failed and n > 1:
            self._dp_iteration(False)                               # one eager iteration: warms RCCL and every lazy initialisation
            n -= 1
            ok, g = 1, None
            try:
                g = self._dp_capture()
            except Exception as e:      # pragma: no cover - depends on the RCCL / driver stack
                logging.warning("rank %s: data-parallel iteration could not be captured into a graph (%s)", self._rank(), e)
                ok = 0
                torch.cuda.synchronize()
            if comm:
                flag = torch.tensor([ok], device=self.dev, dtype=torch.int32)
                dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=self.group)
                ok = int(flag.item())
            if ok:
                self._dp_graph, self._hb_issued = g, 0
                self._hb_dev.zero_()
                self._hb_host.zero_()
            else:
                self._dp_graph_failed = True
                self.dp_fallbacks += 1
                del g
        path = "graph" if self._dp_graph is not None else "host"
        if self.dp_path != path:
            self.dp_path = path
            logging.getLogger("rdo_ptq.dp").info("rank %s: data-parallel loop = %s (world %d)", self._rank(), path, self.world)
        if self._dp_graph is not None:
            for _ in range(n):
                self._dp_graph.replay()
                self._hb_issued += 1
                if self._hb_issued % self.DP_HB_BATCH == 0:         # at most two batches queued: the GPU stays fed, a hang is seen
                    self._hb_wait(self._hb_issued - self.DP_HB_BATCH)
            return
        merge = self.use_graph and os.environ.get("RDO_DP_MERGE", "1") != "0"
        for i in range(n):
            self._dp_iteration(self.use_graph, first=(i == 0 or not merge), last=(i == n - 1 or not merge))

    def _rank(self):
        dist = torch.distributed
        return dist.get_rank(self.group) if (dist.is_available() and dist.is_initialized()) else 0
