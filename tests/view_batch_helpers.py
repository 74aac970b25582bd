"""Plumbing of the view-batch tests (tests/test_cpu_view_batch.py, tests/test_gpu_view_batch.py): `multiview_batch_step`
under every schedule of its pipeline, every view checked against ITS OWN float32 oracle gradients.

The one existing GPU test of the batch step builds its expectation from clones of the bucket taken when a view is packed:
a view whose rows were overwritten too early (the hazard the `bucket_free` event exists to prevent) is wrong in the clone
and in the message alike.  Here the clones are compared with the oracle of that view, so such a view fails by orders of
magnitude; the product is never its own reference for a gradient.

Reference: per view, `oracle_forward` / `oracle_backward` of tests/helpers.py on `make_case(..., view=v, nviews=K)`, cached
once per (case, view, step) and never modified; the batch reference is the float64 sum of those in ascending view order,
the radii reference their maximum.  Plain helpers, no fixtures: the backend (the HIP library, or the oracle backend a CPU
test installs) is whatever `gaussianeditor_amd.multiview._C` is when a `Runner` is used."""
import contextlib
import functools

import numpy as np
import torch

from helpers import assert_grads_close, make_case, oracle_backward, oracle_forward, seed_gradient, settings

#: the smallest shapes that still exercise the code: ragged edge tiles (100 x 75 is 7 x 5 tiles of 16), three 1024-row
#: header blocks of the view messages at P = 2500, one row in the second block at P = 1025, a single Gaussian at P = 1
W, H, M, D, S0, SEED = 100, 75, 16, 3, 0.04, 4
P_MAIN, P_EDGE, P_ONE = 2500, 1025, 1
TOL = 1e-5  # the project's bar (helpers.assert_grads_close adds the per-row bars)
OVERFLOW_HINT = 16  # the third step speculates on 16 rows: every view with more touched rows overflows it
SEG_KEYS = ("dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dmeans2D", "dL_dopacity")  # multiview._ROW_SEGS, oracle names
GRAD_KEYS = SEG_KEYS + ("dL_dsh",)

#: name -> the module attributes of gaussianeditor_amd.multiview that select it (GSR_VIEW_PIPELINE / _AHEAD / _AUTOGRAD)
SCHEDULES = {
    "serial": dict(_VIEW_PIPELINE=False, _VIEW_AHEAD=0, _VIEW_AUTOGRAD=False),
    "ahead0": dict(_VIEW_PIPELINE=True, _VIEW_AHEAD=0, _VIEW_AUTOGRAD=False),
    "ahead1": dict(_VIEW_PIPELINE=True, _VIEW_AHEAD=1, _VIEW_AUTOGRAD=False),
    "ahead2": dict(_VIEW_PIPELINE=True, _VIEW_AHEAD=2, _VIEW_AUTOGRAD=False),
    "autograd": dict(_VIEW_PIPELINE=True, _VIEW_AHEAD=0, _VIEW_AUTOGRAD=True),
}


def _oracle():
    from oracle import cpu

    cpu.build()
    return cpu


# ---- the cases and their reference (computed once, shared, left unchanged) -------------------------------------------
@functools.lru_cache(maxsize=None)
def view_case(P, K, v, away=False):
    """View `v` of the K-view ring around the scene of P Gaussians; `away`: the same camera position, turned round, so that
    the whole cloud lies behind it."""
    case = make_case(P, W, H, seed=SEED, s0=S0, view=v, nviews=K, sh_degree=D)
    if away:
        from gaussianeditor_amd.synth import look_at_camera

        eye = case["cam"].camera_center.double().numpy()
        case["cam"] = look_at_camera(eye, 2.0 * eye, W, H)
    return case


def pixel_gradient(v, step):
    """dL/dcolor of view `v` in step `step`: another seed per view and per step."""
    return seed_gradient(H, W, 100 + v + 1000 * step) * H * W


@functools.lru_cache(maxsize=None)
def oracle_view_forward(P, K, v, away=False):
    return oracle_forward(_oracle(), view_case(P, K, v, away))


@functools.lru_cache(maxsize=None)
def oracle_view_grads(P, K, v, away, step):
    """-> (the six float32 oracle gradients of the view, (P, -1) each; the rows the blend backward adds to, bool (P,))."""
    case = view_case(P, K, v, away)
    g = oracle_backward(_oracle(), case, oracle_view_forward(P, K, v, away), pixel_gradient(v, step))
    grads = {k: np.ascontiguousarray(g[k]).reshape(P, -1) for k in GRAD_KEYS}
    rows = np.concatenate([np.ascontiguousarray(g[k]).reshape(P, -1) for k in ("dL_dmeans2D", "dL_dopacity", "dL_dconic", "dL_dcolors")],
                          axis=1)
    for a in grads.values():
        a.setflags(write=False)
    return grads, (rows != 0).any(axis=1)


class Batch:
    """K views of one scene; `away`: the views whose camera is turned away from the cloud."""

    def __init__(self, P, K, away=()):
        self.P, self.K, self.away = int(P), int(K), tuple(away)
        self.specs = [(self.P, self.K, v, v in self.away) for v in range(self.K)]

    def cases(self):
        return [view_case(*s) for s in self.specs]

    def params(self, dev):
        sc = self.cases()[0]["sc"]
        return {k: sc[k].to(dev).contiguous() for k in ("xyz", "opacity", "features", "scaling", "rotation")}

    def oracle(self, v, step):
        return oracle_view_grads(*self.specs[v], step)

    def oracle_radii(self):
        return np.maximum.reduce([oracle_view_forward(*s)["radii"] for s in self.specs])


#: every batch the GPU tests run, as (P, K, away): tests/test_cpu_view_batch.py establishes from the oracle alone that they meet
#: the tests' conditions
ALL_BATCHES = [(P_MAIN, K, ()) for K in (1, 2, 3, 5, 9)] + [(P_EDGE, 3, ()), (P_ONE, 3, ()), (P_MAIN, 3, (1,)), (P_MAIN, 3, (1, 2)),
                                                                   (P_MAIN, 3, (0, 1, 2))]


def message_rows(message, P):
    """-> (count, the row numbers) of a packed view message (include/gsr.h: word 3, then 4 + ceil(P / 1024) header words)."""
    w = message.detach().cpu().view(torch.int32)
    n, head = int(w[3]), 4 + (int(P) + 1023) // 1024
    return n, w[head:head + n].to(torch.int64)


def next_hint(counts):
    """What a step leaves for the next one to speculate on: ceil(1.5 max(counts, 1) / 1024) 1024, in integers."""
    return -(-3 * max(max(counts), 1) // 2048) * 1024


# ---- the recorder ----------------------------------------------------------------------------------------------------
class Spy:
    """Records, per `_batch_step` pass (a discarded speculative pass is one), what every view handed to the pack kernel --
    clones of the five row segments, `rgb`, `campos`, taken on the stream the pack runs on -- and the flags of every render;
    and every PendingForward `rasterize_gaussians_begin` handed out."""

    def __init__(self, monkeypatch, mv):
        from gaussianeditor_amd import options

        self.passes, self.pending, self.active = [], [], None
        C = mv._C
        orig_step, orig_pack = mv._batch_step, C.view_message_pack
        orig_begin, orig_render = getattr(C, "rasterize_gaussians_begin", None), C.rasterize_gaussians

        def batch_step(*a):
            rec = dict(spec_cap=a[6], packs=[], renders=[], discarded=None)
            self.passes.append(rec)
            self.active = rec
            try:
                out = orig_step(*a)
                rec["discarded"] = out is None
                return out
            finally:
                self.active = None

        def pack(plan, grads5, rgb, campos, cap, message):
            if self.active is not None:
                self.active["packs"].append(dict(g5=[g.clone() for g in grads5], rgb=rgb.clone(), campos=campos.clone(),
                                                 cap=int(cap), message=message))
            return orig_pack(plan, grads5, rgb, campos, cap, message)

        def flags_of(kw):
            return options.current_flags() if kw.get("flags") is None else int(kw["flags"])

        def begin(*a, **kw):
            if self.active is not None:
                self.active["renders"].append(("begin", flags_of(kw)))
            pf = orig_begin(*a, **kw)
            self.pending.append(pf)
            return pf

        def render(*a, **kw):
            if self.active is not None:
                self.active["renders"].append(("whole", flags_of(kw)))
            return orig_render(*a, **kw)

        monkeypatch.setattr(mv, "_batch_step", batch_step)
        monkeypatch.setattr(C, "view_message_pack", pack)
        monkeypatch.setattr(C, "rasterize_gaussians", render)
        if orig_begin is not None:
            monkeypatch.setattr(C, "rasterize_gaussians_begin", begin)


# ---- one bucket, several steps -----------------------------------------------------------------------------------------
class Runner:
    """Steps `multiview_batch_step` on ONE bucket under one schedule and checks every step (module docstring).  `ratios`
    collects the worst per-view and batch-sum errors, each as a fraction of its bar."""

    def __init__(self, monkeypatch, batch, dev, schedule, bucket_kw=None, caller_flags=None, oracle_checks=True):
        from gaussianeditor_amd import multiview as mv
        from gaussianeditor_amd import options

        self.mv, self.options, self.batch, self.dev, self.schedule = mv, options, batch, torch.device(dev), schedule
        for name, value in SCHEDULES[schedule].items():
            monkeypatch.setattr(mv, name, value)
        self.spy = Spy(monkeypatch, mv)
        self.params = batch.params(dev)
        self.settings = [settings(c, dev) for c in batch.cases()]
        self.bucket = mv.GradBucket(batch.P, M, self.dev, sh_exchange="rgb", **(bucket_kw or {}))
        # check 4: whatever the step does not write stays NaN
        self.bucket._buf.fill_(float("nan"))
        self.bucket.rgb.fill_(float("nan"))
        self.caller_flags = caller_flags  # flags the caller has set with options.override around the step (None: none)
        self.oracle_checks = oracle_checks  # (off under FLAG_FAST_EXP: another exp, not the oracle's arithmetic)
        self.ratios = dict(view=0.0, sum=0.0)
        self.forwards = None

    # the views' own forwards: no-grad renders on the default stream, once (they do not depend on the step)
    def _reference_forwards(self):
        if self.forwards is None:
            from gaussianeditor_amd.diff_gaussian_rasterization import GaussianRasterizer

            p = self.params
            with torch.no_grad():
                self.forwards = [GaussianRasterizer(s)(p["xyz"], torch.zeros_like(p["xyz"]), p["opacity"], shs=p["features"],
                                                       scales=p["scaling"], rotations=p["rotation"]) for s in self.settings]
        return self.forwards

    def sync(self):
        if self.dev.type == "cuda":
            torch.cuda.synchronize(self.dev)

    def call(self, step):
        """The product call alone, inside the caller's flag override."""
        Gs = [pixel_gradient(v, step).to(self.dev).contiguous() for v in range(self.batch.K)]
        ctx = self.options.override(self.caller_flags) if self.caller_flags is not None else contextlib.nullcontext()
        with ctx:
            before = self.options.current_flags()
            try:
                return self.mv.multiview_batch_step(self.settings, self.params, Gs, self.bucket)
            finally:
                after = self.options.current_flags()
                assert after == before, (self.schedule, step, "the thread's flags were not restored", before, after)

    def compose(self, pk):
        P = self.batch.P
        return self.mv._C.sh_grad_compose(self.params["xyz"], pk["campos"].view(1, 3), pk["rgb"].view(1, P, 3), D, M)

    def step(self, step, cap_hint=None, must_overflow=None):
        """One step and its checks -> the step's passes (the last one produced the result)."""
        mv, spy, bucket, batch = self.mv, self.spy, self.bucket, self.batch
        P, K = batch.P, batch.K
        tag = f"{self.schedule} K={K} P={P} step {step}"
        self._reference_forwards()
        if bucket.row_state is not None:
            bucket.check_persistent_rows()
        if cap_hint is not None:
            bucket._cap_hint = cap_hint
        hint = bucket._cap_hint
        flags_before = self.options.current_flags()
        first = len(spy.passes)
        colors, radii, depths, grads = self.call(step)
        self.sync()
        assert self.options.current_flags() == flags_before and bucket.on_blend_done is None, tag
        passes = spy.passes[first:]
        last = passes[-1]
        counts = list(bucket.last_counts)
        # ---- the speculation's arithmetic, and which passes ran
        assert len(counts) == K and bucket.last_route == "rows", tag
        for v, pk in enumerate(last["packs"]):
            assert message_rows(pk["message"], P)[0] == counts[v], (tag, v, "the message header's count")
        overflow = hint is not None and max(counts) > hint
        if must_overflow is not None:
            assert overflow == must_overflow, (tag, hint, counts)
        want_passes = [None] if hint is None else ([hint, None] if overflow else [hint])
        assert [p["spec_cap"] for p in passes] == want_passes, (tag, [p["spec_cap"] for p in passes], want_passes)
        assert [p["discarded"] for p in passes] == [True, False][-len(passes):], tag
        ex = bucket.last_exchange
        assert ex["speculated"] is (hint is not None and not overflow), (tag, ex)
        assert ex["message_rows"] == (hint if ex["speculated"] else max(max(counts), 1)), (tag, ex, counts)
        assert ex["views"] == K and ex["views_local"] == K and ex["bytes_sent"] == 0, (tag, ex)
        assert bucket._cap_hint == next_hint(counts), (tag, bucket._cap_hint, counts)
        # ---- check 5: the flags of every render
        caller = flags_before if self.caller_flags is None else self.caller_flags
        shared = self.options.FLAG_SHARED_SIMDS
        for p in passes:
            assert len(p["packs"]) == K and len(p["renders"]) == K, (tag, len(p["packs"]), len(p["renders"]))
            pipelined = (p["spec_cap"] is not None and K > 1 and self.schedule != "serial" and self.dev.type == "cuda")
            whole = not pipelined or self.schedule == "autograd"
            for kind, flags in p["renders"]:
                assert kind == ("whole" if whole else "begin"), (tag, kind)
                assert flags == (caller | shared if pipelined else caller), (tag, kind, flags, caller, pipelined)
        # ---- check 1: every view on its own, against its own oracle gradients (the discarded pass's views too)
        if self.oracle_checks:
            for p in passes:
                for v, pk in enumerate(p["packs"]):
                    want, _ = batch.oracle(v, step)
                    got = {k: t.detach().cpu().numpy() for k, t in zip(SEG_KEYS, pk["g5"])}
                    got["dL_dsh"] = self.compose(pk).cpu().numpy()
                    worst = assert_grads_close(got, want, tol=TOL, tag=f"{tag} view {v}" + (" (discarded pass)" if p["discarded"] else ""))
                    self.ratios["view"] = max(self.ratios["view"], worst / TOL)
        # ---- check 2: the sums -- bit-equal to the captured views added in view order ...
        packs = last["packs"]
        tot, sh = [t.clone() for t in packs[0]["g5"]], self.compose(packs[0])
        for pk in packs[1:]:
            tot = [a + b for a, b in zip(tot, pk["g5"])]
            sh = sh + self.compose(pk)
        valid = None if bucket.row_valid is None else bucket.row_valid.bool()
        got_sums = dict(zip(SEG_KEYS, (bucket.views[name] for name in mv._ROW_SEGS)), dL_dsh=bucket.views["sh"])
        assert grads["sh"] is bucket.views["sh"] and tuple(bucket.views["sh"].shape) == (P, M, 3), tag
        for key, want_t in zip(GRAD_KEYS, tot + [sh]):
            a, b = got_sums[key].reshape(P, -1), want_t.reshape(P, -1)
            if valid is not None:  # sparse rows: only the rows some view sent are written
                a, b = a[valid], b[valid]
            assert torch.equal(a, b), (tag, key, "not the sequential sum of the views as they were packed")
        # ... and close to the float64 sum of the views' oracle gradients: the per-view bar added up
        if self.oracle_checks:
            for key in GRAD_KEYS:
                ref, bound = np.zeros((P, got_sums[key].numel() // P)), 0.0
                for v in range(K):
                    g = batch.oracle(v, step)[0][key].astype(np.float64)
                    ref += g
                    bound += TOL * float(np.abs(g).max())
                a = got_sums[key].detach().cpu().numpy().astype(np.float64).reshape(ref.shape)
                if valid is not None:
                    a = np.where(valid.cpu().numpy()[:, None], a, 0.0)  # (rows that are not valid count as zeros)
                err = float(np.abs(a - ref).max())
                assert err <= bound, (tag, key, err, bound)
                if bound > 0:
                    self.ratios["sum"] = max(self.ratios["sum"], err / bound)
        # ---- check 3: the forward outputs do not depend on the schedule
        assert len(colors) == K and len(depths) == K, tag
        rad = None
        for v, (c, r, d_) in enumerate(self.forwards):
            assert torch.equal(colors[v], c), (tag, v, "colour", float((colors[v] - c).abs().max()))
            assert torch.equal(depths[v], d_), (tag, v, "depth", float((depths[v] - d_).abs().max()))
            rad = r.clone() if rad is None else torch.maximum(rad, r)
        assert torch.equal(radii, rad), (tag, "radii")
        assert np.array_equal(radii.cpu().numpy(), batch.oracle_radii()), (tag, "radii against the oracle")
        # ---- check 4: nothing left unwritten
        for name, t in list(bucket.views.items()) + [("rgb", bucket.rgb)]:
            t = t.reshape(P, -1)
            if valid is not None and name != "rgb":
                t = t[valid]  # (sparse rows: the exchange writes no other row, see the sparse test)
            assert bool(torch.isfinite(t).all()), (tag, name, "holds entries no kernel wrote")
        return passes

    def four_steps(self, may_overflow=True):
        """The sequence every schedule runs: exact, speculated, overflowing (hint 16), speculated."""
        out = [self.step(0)]
        assert out[0][-1]["spec_cap"] is None
        out.append(self.step(1))
        out.append(self.step(2, cap_hint=OVERFLOW_HINT, must_overflow=may_overflow))
        assert self.bucket.last_exchange["speculated"] is (not may_overflow)
        out.append(self.step(3))
        assert self.bucket.last_exchange["speculated"] is True
        return out

    def report(self, what=""):
        print(f"[view batch {self.schedule} K={self.batch.K} P={self.batch.P}{what}] worst per-view error {self.ratios['view']:.3f} "
              f"of the 1e-5 bar, worst batch-sum error {self.ratios['sum']:.3f} of its bar")

