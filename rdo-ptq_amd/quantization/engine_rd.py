"""The opt-in R + lambda*D task loss of a unit (loss_mode='rd'): which modules of the wrapped model do not depend on the unit (evaluated
once per calibration image), the model tail on torch's tape, and the loop that drives plan A -> tail -> plan RD.  A base class of
`engine.UnitEngine`; it never touches a kernel helper."""
import contextlib
import logging
import os

import torch

from hipops import _lib as L


@contextlib.contextmanager
def forwards(fwd):
    """Install `fwd` ({module: function}) as the modules' `forward` INSTANCE attributes for the block and delete them behind it, so
    that the classes' forwards answer again (nothing is saved and restored: a module that carried a forward of its own loses it)."""
    done = []
    try:
        for m, f in fwd.items():
            m.forward = f
            done.append(m)
        yield
    finally:
        for m in done:
            del m.forward


class RdTask:
    """The R + lambda*D mode of `UnitEngine`: `rd` = dict(model=QuantModel, unit=module, cali=calibration images NCHW on the GPU,
    lmbda=float, metric='mse' | 'ms-ssim' (optional, default 'mse')).  The unit output of every iteration is pushed through the REST
    of the wrapped model on torch's tape (hipops.autograd) and losses.RateDistortionLoss is differentiated back to it; rec_loss stays
    the lp term.

    Reads of the engine: `plan_a`, `plan_rd`, `plan_b` (the recorded plans), `_rd_pred` and `g_task` (the unit output and the buffer
    of its task gradient, set by the recording: `UnitEngine._loss`), `it`, `idx`, `task_log`, `B`, `split`, `bucket`, `use_graph`, `dev`.
    Owns: `rd` (with its keys 'memo' and 'skip'), `rd_path`, `_rd_graph`, `_rd_graph_failed`.  The engine drops `_rd_graph` when it
    records its plans anew (`_recover`) and the memo when the unit is finished."""

    def _rd_init(self, rd, include_act_func):
        self.rd = rd
        self.rd_path = None                    # "graph" | "host" once an R + lambda*D run has started (_run_rd)
        self._rd_graph, self._rd_graph_failed = None, False
        if rd is None:
            return
        metric = rd.get("metric", "mse")
        if metric not in ("mse", "ms-ssim"):
            raise ValueError(f"loss_mode='rd': unknown metric {metric!r} ('mse' or 'ms-ssim')")
        if metric == "ms-ssim" and min(rd["cali"].shape[-2:]) <= 160:
            raise ValueError(f"loss_mode='rd' with metric 'ms-ssim' needs calibration crops with both sides above 160 pixels (five "
                             f"scales of an 11-tap window); got {tuple(rd['cali'].shape[-2:])}")
        if not include_act_func:
            raise NotImplementedError("calibration engine: loss_mode='rd' substitutes the unit's module OUTPUT (after its fused "
                                      "activation); include_act_func=False optimises the pre-activation and cannot be combined with it")

    def _rd_iteration(self, graph):
        """One iteration of the R + lambda*D mode on the current stream: plan A (gather, unit forward, rec_loss and its gradient) ->
        the task term (the whole model behind the unit, `_rd_tail`) -> plan RD (+ g_task, backward, AdaRound step -- or, data
        parallel, the gradient bucket) [-> all-reduce -> plan B]."""
        self.plan_a.run(1, graph=graph)
        self._rd_tail()
        self.plan_rd.run(1, graph=graph)
        if self.split:
            self.bucket.reduce()
            self.plan_b.run(1, graph=graph)

    def _run_rd(self, n):
        """n iterations of the R + lambda*D mode.  Single process with graphs on: the WHOLE iteration -- the recorded kernels of both
        plans and the model tail with its autograd backward (every op of which is a device-side kernel: the mini-batch rows are
        selected with the device iteration counter) -- is captured once into one graph (torch.cuda.graph) and replayed, no host work
        per iteration.  `RDO_RD_GRAPH=0`, a refused capture, or the data-parallel split (a collective per iteration): host-driven."""
        want = self.use_graph and not self.split and os.environ.get("RDO_RD_GRAPH", "1") != "0"
        if want and self._rd_graph is None and not self._rd_graph_failed and n > 2:
            self._rd_iteration(False)                 # eager: every lazy initialisation (scratch buffers, kernel attributes, autograd)
            n -= 1
            torch.cuda.synchronize()
            try:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._rd_iteration(False)
                self._rd_graph = g
            except Exception as e:      # pragma: no cover - depends on the driver stack
                logging.warning("R + lambda*D iteration could not be captured into a graph (%s): host-driven loop", e)
                self._rd_graph_failed = True
                torch.cuda.synchronize()
        self.rd_path = "graph" if self._rd_graph is not None else "host"
        if self._rd_graph is not None:
            for _ in range(n):
                self._rd_graph.replay()
            return
        for _ in range(n):
            self._rd_iteration(self.use_graph)

    # ---- what does not depend on this unit is computed once per calibration image --------------------------------------------------
    RD_CACHE_LIMIT = 8 << 30            # bytes of cached module outputs per unit (a coder's latent for 256 images is 50-100 MB)

    @staticmethod
    def _tree(fn, t):
        if torch.is_tensor(t):
            return fn(t)
        if isinstance(t, dict):
            return {k: RdTask._tree(fn, v) for k, v in t.items()}
        if isinstance(t, (tuple, list)):
            return type(t)(RdTask._tree(fn, v) for v in t)
        return t

    def _rd_cut(self, unit_forward):
        """{module: forward} that takes the unit out of the model: `unit_forward` in its place, what only feeds it passed through"""
        return {self.rd["unit"]: unit_forward, **{m: (lambda x, *a, **k: x) for m in self.rd["skip"]}}

    def _rd_prepare(self):
        """Modules of the wrapped model whose INPUTS do not depend on this unit's output produce the same output for an image in every
        iteration (weights behind and before the unit are fixed for the unit's run): found by running the model twice on one
        mini-batch with two different random tensors in place of the unit's output, on torch's tape: a candidate is independent when
        its inputs are bit-equal in both runs AND none of them carries a grad_fn back to the substituted tensor (values alone are not
        enough: two different hyper-latents can round to the same z^; the tape alone is not either: a detached activation
        quantiser cuts it).  Independent modules are evaluated ONCE per calibration image (in mini-batches of B, the shape the iterations run at) and looked up by row afterwards.
        Candidates: the children of the model (the coders and entropy models) that do not contain the unit.  Inside the coder that
        does, the modules in front of the unit in an nn.Sequential only feed the unit, whose forward is replaced: they are skipped.
        A candidate holding a live dynamic activation quantiser (statistics over the mini-batch) is left alone.  `RDO_RD_CACHE=0`
        turns all of this off."""
        rd = self.rd
        rd["memo"], rd["skip"] = {}, []
        if os.environ.get("RDO_RD_CACHE", "1") == "0":
            return
        from .quant_block import BaseQuantBlock
        from .quant_layer import QuantModule
        model, unit, cali = rd["model"], rd["unit"], rd["cali"]
        root = model.model if isinstance(getattr(model, "model", None), torch.nn.Module) else model
        holds = lambda m: any(c is unit for c in m.modules())
        cands = []
        for _, child in root.named_children():
            if not holds(child):
                cands.append(child)
                continue
            box = child
            while box is not unit and isinstance(box, torch.nn.Sequential):       # descend to the unit: skip what only feeds it
                kids = list(box.children())
                k = next(i for i, c in enumerate(kids) if holds(c))
                rd["skip"] += kids[:k]
                box = kids[k]
        live_aq = lambda m: any(isinstance(c, (QuantModule, BaseQuantBlock)) and c.use_act_quant and c.trained
                                and not getattr(c, "disable_act_quant", False) for c in m.modules())
        cands = [c for c in cands if not live_aq(c)]
        if not cands:
            return
        was_training = model.training
        model.eval()
        B = self.B
        shape = tuple(self._rd_pred.permute(0, 3, 1, 2).shape)
        seen = [{}, {}]
        try:
            tainted = set()

            def note(m, a, k, run):
                flag = [False]
                self._tree(lambda t: flag.__setitem__(0, flag[0] or t.requires_grad), (a, k))
                if flag[0] or id(m) in seen[run]:
                    # depends on the unit -- or is called more than once per model forward (a shared / looped module): its outputs
                    # could not be told apart by image row, so it is never memoised
                    tainted.add(id(m))
                seen[run][id(m)] = self._tree(lambda t: t.detach().clone(), (a, k))
            for run in range(2):
                fake = torch.randn(shape, device=self.dev, generator=torch.Generator(device=self.dev).manual_seed(17 + run)).requires_grad_(True)
                hooks = [c.register_forward_pre_hook(lambda m, a, k, run=run: note(m, a, k, run), with_kwargs=True) for c in cands]
                try:
                    with forwards(self._rd_cut(lambda *a, fake=fake, **k: fake)), torch.enable_grad():
                        model(cali[:B])
                finally:
                    for h in hooks:
                        h.remove()
            with torch.no_grad():

                def same(a, b):
                    if torch.is_tensor(a):
                        return torch.is_tensor(b) and a.shape == b.shape and bool(torch.equal(a, b))
                    if isinstance(a, dict):
                        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
                    if isinstance(a, (tuple, list)):
                        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
                    return a == b
                free = [c for c in cands if id(c) in seen[0] and id(c) in seen[1] and id(c) not in tainted and same(seen[0][id(c)], seen[1][id(c)])]
                seen = None
                if not free:
                    return
                # one pass over the calibration images: outputs of the unit-independent modules, image-major
                parts = {id(c): [] for c in free}
                hooks = [c.register_forward_hook(lambda m, a, o: parts[id(m)].append(self._tree(lambda t: t.detach().clone(), o))) for c in free]
                try:
                    with forwards(self._rd_cut(lambda *a, **k: torch.zeros(shape, device=self.dev))):
                        n = cali.shape[0]
                        n_fwd = 0
                        for i in range(0, n, B):
                            xb = cali[i:i + B]
                            if xb.shape[0] < B:                               # ragged end: pad the mini-batch with the first images
                                xb = torch.cat([xb, cali[:B - xb.shape[0]]])
                            model(xb)
                            n_fwd += 1
                finally:
                    for h in hooks:
                        h.remove()

                def cat(chunks):
                    first = chunks[0]
                    if torch.is_tensor(first):
                        return torch.cat(chunks)[:n] if first.dim() > 0 and first.shape[0] == B else None
                    if isinstance(first, dict):
                        out = {k: cat([c[k] for c in chunks]) for k in first}
                        return None if any(v is None for v in out.values()) else out
                    if isinstance(first, (tuple, list)):
                        out = [cat([c[j] for c in chunks]) for j in range(len(first))]
                        return None if any(v is None for v in out) else type(first)(out)
                    return None
                total = 0
                for c in free:
                    chunks = parts.pop(id(c))
                    if len(chunks) != n_fwd:                                  # exactly one call per model forward, or the rows of the
                        continue                                              # concatenation would not be the calibration images
                    memo = cat(chunks)
                    if memo is None:
                        continue                                              # an output that is not per-image: leave the module alone
                    nbytes = [0]
                    self._tree(lambda v: nbytes.__setitem__(0, nbytes[0] + v.numel() * v.element_size()), memo)
                    if total + nbytes[0] > self.RD_CACHE_LIMIT:
                        continue
                    total += nbytes[0]
                    rd["memo"][c] = memo
        finally:
            model.train(was_training)

    def _rd_tail(self):
        """The current iteration's task loss: the images of the mini-batch through the wrapped model with this unit's output replaced
        by the engine's soft-quantised output, `RateDistortionLoss` (lambda * 255^2 * MSE + bpp, or lambda * (1 - MS-SSIM) + bpp with
        rd['metric'] = 'ms-ssim') on the result, gradient back to that
        output (HIP kernels under torch's tape: hipops.autograd; the factorised prior and the Gaussian conditional included).  The
        modules behind the unit are whatever the calibration flow left them: trained ones hard-quantised, the others full precision
        (layer_opt.py:15-43).  Device-side throughout (capturable): the mini-batch rows come from the index table through the device
        iteration counter."""
        from losses.losses import RateDistortionLoss
        rd = self.rd
        it = self.it.long()                                                   # [1], published by this iteration's gather
        rows = self.idx.index_select(0, it).view(-1).long()
        x = rd["cali"].index_select(0, rows)
        leaf = self._rd_pred.permute(0, 3, 1, 2).detach().requires_grad_(True)
        if "memo" not in rd:
            self._rd_prepare()
        was_training = rd["model"].training
        rd["model"].eval()
        fwd = self._rd_cut(lambda *a, **k: leaf)       # the unit itself is not run: its output is the engine's -- nor what only feeds it
        for m_, memo in rd["memo"].items():            # ... and what does not depend on it is looked up per image
            fwd[m_] = lambda *a, memo=memo, **k: self._tree(lambda t: t.index_select(0, rows), memo)
        try:
            with forwards(fwd), torch.enable_grad():
                out = rd["model"](x)
                loss = RateDistortionLoss(lmbda=rd["lmbda"], metric=rd.get("metric", "mse"))(out, x)["loss"]
                # (a tape cut on EVERY path from the unit's output leaves a loss without a grad_fn: the same finding as a gradient of None)
                g = torch.autograd.grad(loss, [leaf], allow_unused=True)[0] if loss.requires_grad else None
        finally:
            rd["model"].train(was_training)
        if g is None:
            raise RuntimeError("loss_mode='rd': no gradient reached the unit's output -- a module behind it detaches the tape (dynamic "
                               "activation quantisers of trained modules do); run the RD task loss with act_quant=False")
        self.g_task.copy_(g.permute(0, 2, 3, 1))
        self.task_log.view(-1).index_add_(0, it * L.LOG_SLOTS, loss.detach().reshape(1))
