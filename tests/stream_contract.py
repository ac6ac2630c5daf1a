"""The stream contract of the device-pointer entry points of include/sfb.h, and the harness that tests it
(tests/test_stream_contract_gpu.py).

The contract: an entry called with `stream` (1) reads its inputs behind the work already enqueued on `stream`, (2) has every
output and in-out buffer complete for whatever is enqueued on `stream` afterwards, and (3) takes and releases its temporary
memory in stream order.  On the null stream, or between device-wide synchronisations, a launch, memset or helper on the wrong
stream still gives the right answer; so every case here runs on NON-BLOCKING side streams, behind a bounded spin
(torch.cuda._sleep), with its inputs arriving on that stream after the spin and its outputs read by copies on that stream
and nothing else.

A case is a pair of Jobs with equal shapes: the real problem and a decoy (valid data of the same kind: another seed of the
generator, another level or the neighbouring rows of a fixture -- never NaN, never an index out of range).  run_case does, for
one case:
  1. baseline: the real job twice on the null stream, equal bit for bit, and within the entry's own test's comparison against
     its independent reference (oracle, *_ref.py restatement or fixture gate); the decoy job once;
  2. warm-up: each job on its side stream, ungated (slot creation, module load, LDS opt-in), equal to its baseline; a second
     ungated call of the real job is timed on the host: the enqueue time that sizes the spin;
  3. ordered run: the buffers hold the decoy and sentinels; on s: spin, device-to-device copies of the real inputs, the entry,
     copies of every output and in-out buffer to snapshots; pending = not s.query() right after; s.synchronize() only; the
     snapshots equal the baseline;
  4. two streams: the real job on s1 and the decoy job (own buffers, workspace, outputs) on s2, each as in 3, enqueued back to
     back; each equals its own baseline.
Entries whose results hold device-clock times (the TIME column of a trace, phase_us) are compared through Job.normalize, which
drops those and checks them by the gate of their existing test instead.
"""
import ctypes as C
import os
import re
import time
from dataclasses import dataclass, field
from typing import Callable, Dict, Optional, Tuple

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sfb.h")

# Not covered, for the record (neither takes a `void *stream`, so the coverage test never sees them): sfb_mpc_swarm_step_resident
# and sfb_mpc_swarm_upload work on the null stream and on the swarm's own copy stream.

SPIN_MIN_MS, SPIN_MAX_MS, SPIN_MARGIN = 20.0, 250.0, 10.0
HIP_STREAM_NON_BLOCKING = 0x01


def header_stream_entries(path=HEADER):
    """names of the functions declared in sfb.h whose parameter list holds `void *stream`"""
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return sorted(m.group(1) for m in re.finditer(r"\bsfb_status\s+(sfb_\w+)\s*\(([^;{]*)\)\s*;", text) if re.search(r"void\s*\*\s*stream\b", m.group(2)))


# ------------------------------------------------------------------------------------------------ jobs
@dataclass
class Job:
    """one problem of a case.  inputs / inout: name -> host array; outputs: name -> (shape, dtype); call(ptr, stream): the
    entry on device pointers (ptr: name -> int) and a hipStream_t handle (int, 0 = null stream); check(result): the baseline
    against the independent reference; normalize(result) -> what is compared bit for bit (after checking the rest)."""
    inputs: Dict[str, np.ndarray]
    inout: Dict[str, np.ndarray]
    outputs: Dict[str, Tuple[tuple, type]]
    call: Callable
    check: Optional[Callable] = None
    normalize: Optional[Callable] = None
    keep: list = field(default_factory=list)     # whatever must outlive the calls (plans, workspaces, groups)


def _sentinel(torch, shape, dtype, dev):
    if np.issubdtype(np.dtype(dtype), np.floating):
        return torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
    return torch.full(shape, -1, dtype=torch.int32, device=dev)


class DeviceJob:
    """the device side of one Job: the buffers the entry works on, device copies of the job's own inputs (the sources of the
    copies on the side stream) and the snapshots"""

    def __init__(self, job, torch):
        self.job, self.torch, self.dev = job, torch, torch.device("cuda:0")
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)        # noqa: E731
        self.src = {k: T(v) for k, v in {**job.inputs, **job.inout}.items()}
        self.buf = {k: torch.empty_like(v) for k, v in self.src.items()}
        for k, (shape, dtype) in job.outputs.items():
            self.buf[k] = _sentinel(torch, shape, dtype, self.dev)
        self.results = list(job.outputs) + list(job.inout)
        self.snap = {k: torch.empty_like(self.buf[k]) for k in self.results}
        self.ptr = {k: v.data_ptr() for k, v in self.buf.items()}

    def load(self, data):
        """buffers <- the inputs and state of `data` (a Job of the same shapes); outputs and snapshots <- sentinels"""
        for k, v in {**data.inputs, **data.inout}.items():
            assert tuple(v.shape) == tuple(self.buf[k].shape) and self.torch.from_numpy(np.ascontiguousarray(v)).dtype == self.buf[k].dtype, k
            self.buf[k].copy_(self.torch.from_numpy(np.ascontiguousarray(v)))
        for k in self.job.outputs:
            self.buf[k].fill_(float("nan") if self.buf[k].is_floating_point() else -1)
        for k, v in self.snap.items():
            v.fill_(float("nan") if v.is_floating_point() else -1)

    def read(self, which):
        return {k: which[k].cpu().numpy() for k in self.results}


def equal_results(a, b):
    """{name: arrays} equal bit for bit (NaN equal to NaN); -> names that differ"""
    bad = []
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        same = np.array_equal(x, y, equal_nan=True) if np.issubdtype(x.dtype, np.floating) else np.array_equal(x, y)
        if not same:
            bad.append(k)
    return bad


# ------------------------------------------------------------------------------------------------ streams and the gate
_HIP = {}


def hip_runtime():
    """the HIP runtime torch has loaded, through ctypes (the mapped libamdhip64 of this process)"""
    if "lib" not in _HIP:
        path = None
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    path = line.split()[-1]
                    break
        if path is None:
            raise RuntimeError("no libamdhip64 mapped: import torch and touch the device first")
        lib = C.CDLL(path)
        lib.hipStreamGetFlags.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
        lib.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        _HIP["lib"] = lib
    return _HIP["lib"]


def stream_flags(handle):
    flags = C.c_uint(0xFFFFFFFF)
    rc = hip_runtime().hipStreamGetFlags(C.c_void_p(handle), C.byref(flags))
    assert rc == 0, "hipStreamGetFlags: %d" % rc
    return flags.value


@dataclass
class Env:
    """per session: two non-blocking caller streams and the calibration of the spin"""
    torch: object
    s1: object
    s2: object
    cycles_per_ms: float
    how: str


def _non_blocking_stream(torch):
    s = torch.cuda.Stream()
    if stream_flags(s.cuda_stream) == HIP_STREAM_NON_BLOCKING:
        return s, "torch.cuda.Stream()"
    h = C.c_void_p()
    rc = hip_runtime().hipStreamCreateWithFlags(C.byref(h), HIP_STREAM_NON_BLOCKING)
    assert rc == 0 and h.value, "hipStreamCreateWithFlags: %d" % rc
    s = torch.cuda.ExternalStream(h.value)          # (kept for the session: the handle is never destroyed under torch)
    assert stream_flags(s.cuda_stream) == HIP_STREAM_NON_BLOCKING
    return s, "hipStreamCreateWithFlags + ExternalStream"


def _time_spin(torch, cycles):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(int(cycles))
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


_ENV = {}


def env():
    if "env" not in _ENV:
        import torch
        torch.cuda.init()
        torch.zeros(1, device="cuda:0")
        s1, how = _non_blocking_stream(torch)
        s2, _ = _non_blocking_stream(torch)
        torch.cuda._sleep(1000)                     # (loads the spin kernel)
        torch.cuda.synchronize()
        cycles = 1_000_000
        ms = _time_spin(torch, cycles)
        while ms < 5.0 and cycles < 1_000_000_000:  # long enough for the events' resolution; every spin here is bounded
            cycles *= 10
            ms = _time_spin(torch, cycles)
        _ENV["env"] = Env(torch, s1, s2, cycles / ms, how)
        print("stream contract: side streams by %s; spin calibration %d cycles = %.3f ms -> %.0f cycles / ms" % (how, cycles, ms, cycles / ms))
    return _ENV["env"]


def spin_ms(enqueue_ms):
    return min(SPIN_MAX_MS, max(SPIN_MIN_MS, SPIN_MARGIN * enqueue_ms))


# ------------------------------------------------------------------------------------------------ the steps
def _run_ungated(dj, data, stream):
    """`data` loaded, one call of dj's entry on `stream` (None: the null stream) -> (results, host milliseconds of the call)"""
    torch = dj.torch
    dj.load(data)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dj.job.call(dj.ptr, stream.cuda_stream if stream is not None else 0)
    ms = 1e3 * (time.perf_counter() - t0)
    if stream is None:
        torch.cuda.synchronize()
        return dj.read(dj.buf), ms
    stream.synchronize()
    with torch.cuda.stream(stream):
        return dj.read(dj.buf), ms


def _enqueue_gated(dj, stream, cycles):
    """on `stream`, no host wait: spin, the job's own inputs into the buffers, the entry, every result into its snapshot"""
    torch = dj.torch
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(cycles))
        for k, v in dj.src.items():
            dj.buf[k].copy_(v, non_blocking=True)
        dj.job.call(dj.ptr, stream.cuda_stream)
        for k in dj.results:
            dj.snap[k].copy_(dj.buf[k], non_blocking=True)
    return not stream.query()


def _read_snapshots(dj, stream):
    stream.synchronize()                            # the stream only, never the device
    with dj.torch.cuda.stream(stream):
        return dj.read(dj.snap)


def run_case(real, decoy, blocking=False, name=""):
    """steps 1 - 4 for one case; -> dict of the figures (enqueue_ms, spin_ms, pending ...).  Raises AssertionError."""
    e = env()
    torch = e.torch
    norm = real.normalize or (lambda r: r)
    A, D = DeviceJob(real, torch), DeviceJob(decoy, torch)
    # 1. baseline on the null stream
    base, _ = _run_ungated(A, real, None)
    again, _ = _run_ungated(A, real, None)
    if real.check is not None:
        real.check(base)
    base, again = norm(base), norm(again)
    assert not equal_results(base, again), "%s: two runs on the null stream differ in %s" % (name, equal_results(base, again))
    base_d = (decoy.normalize or (lambda r: r))(_run_ungated(D, decoy, None)[0])
    # 2. warm-up on the side streams, ungated
    warm, _ = _run_ungated(A, real, e.s1)
    assert not equal_results(base, norm(warm)), "%s: ungated call on a side stream differs from the baseline in %s" % (name, equal_results(base, norm(warm)))
    warm_d, _ = _run_ungated(D, decoy, e.s2)
    assert not equal_results(base_d, (decoy.normalize or (lambda r: r))(warm_d)), "%s: decoy job, ungated call on the second side stream differs" % name
    timed, enqueue_ms = _run_ungated(A, real, e.s1)
    assert not equal_results(base, norm(timed)), name
    ms = spin_ms(enqueue_ms)
    cycles = ms * e.cycles_per_ms
    fig = dict(case=name, enqueue_ms=enqueue_ms, spin_ms=ms)
    # 3. ordered run: decoy in the buffers, the real inputs arrive behind the spin
    A.load(decoy)
    torch.cuda.synchronize()
    fig["pending"] = _enqueue_gated(A, e.s1, cycles)
    got = norm(_read_snapshots(A, e.s1))
    bad = equal_results(base, got)
    errors = []
    if bad:
        errors.append("step 3, ordered run on a side stream: %s differ from the baseline (stale input, incomplete output or freed scratch)" % bad)
    # 4. two caller streams at once, each job with the other's data in its buffers until its own arrives
    A.load(decoy)
    D.load(real)
    torch.cuda.synchronize()
    p1 = _enqueue_gated(A, e.s1, cycles)
    p2 = _enqueue_gated(D, e.s2, cycles)
    fig["pending_two"] = (p1, p2)
    got_a = norm(_read_snapshots(A, e.s1))
    got_d = (decoy.normalize or (lambda r: r))(_read_snapshots(D, e.s2))
    bad_a, bad_d = equal_results(base, got_a), equal_results(base_d, got_d)
    if bad_a or bad_d:
        errors.append("step 4, two streams at once: job A differs from its baseline in %s, job B in %s" % (bad_a, bad_d))
    # asynchrony and vacuity guard: the call returned, and the snapshots were enqueued, while the spin still held the stream
    if not blocking and not (fig["pending"] and p1 and p2):
        errors.append("the stream had drained when the enqueue returned (pending %s, two streams %s): the entry blocks, or the gate is vacuous" % (fig["pending"], (p1, p2)))
    print("stream contract %-58s enqueue %7.3f ms  spin %6.1f ms  pending %s  two streams pending %s  %s"
          % (name, enqueue_ms, ms, fig["pending"], fig["pending_two"], "FAILED" if errors else "ok"))
    assert not errors, "%s: %s" % (name, "; ".join(errors))
    torch.cuda.synchronize()
    return fig


# ------------------------------------------------------------------------------------------------ case builders
# Each returns (real Job, decoy Job).  The generators, fixtures, references and comparison helpers are those of the entries'
# own tests; nothing here states a tolerance of its own except where said (the 5-knot splines).
def _tile(a, B):
    a = np.asarray(a)
    return np.ascontiguousarray(a[np.arange(B) % len(a)])


def _rolled(arrays):
    """the decoy of fixture rows: every agent carries its neighbour's row (valid data of the same generator, different for every agent)"""
    return {k: np.ascontiguousarray(np.roll(v, 1, axis=0)) for k, v in arrays.items()}


def _qp_outputs(B, n, m):
    return {"x": ((B, n), np.float64), "y": ((B, m), np.float64), "obj": ((B,), np.float64), "iter": ((B,), np.int32), "code": ((B,), np.int32)}


def _qp_solution(sfb, r):
    return sfb.QPBatchSolution(code=r["code"], iter=r["iter"].view(np.uint32), primal=r["x"], dual=r["y"], objective=r["obj"])


def _drop_times(r):
    """trace without its TIME column, no phase_us: what is reproducible of a traced solve; the times are checked for having been
    written (finite, non-negative), as their own tests do"""
    out = dict(r)
    if "trace" in out:
        tr = out["trace"]
        used = tr[:, :, 0] >= 0
        assert np.isfinite(tr[:, :, 4][used]).all() and (tr[:, :, 4][used] >= 0).all(), "TIME column of used rows not written"
        out["trace"] = tr[:, :, :4]
    if "phase_us" in out:
        ph = out.pop("phase_us")[:, :6]
        assert np.isfinite(ph).all() and (ph >= 0).all(), "phase times not written"
    return out


def _dense_data(sfb, n, m, B, seed, recipe):
    if recipe == "big":          # tests/test_qp_dense_gpu.py::test_larger_dense_problems_are_bit_identical_to_the_dense_oracle
        P, q, A, l, u = sfb.random_qp_batch(seed, B, m, n, 0.6)
        rng = np.random.default_rng(seed)
        l = np.where(rng.random((B, m)) < 0.5, u - 1.0 - rng.random((B, m)), l)
        if m > 100:
            u = u + 5.0
            l = np.where(np.isfinite(l), l - 5.0, l)
        return P, q, A, l, u
    return sfb.random_qp_batch(seed, B, m, n, recipe)


def dense_case(sfb, oracle, n, m, B, entry="plain", warm=False, recipe=0.8, max_iter=4000, seeds=(101, 202), rows=10, compare="oracle"):
    from test_qp_dense_gpu import _compare, _compare_full_pattern, _compare_trace, _oracle_params
    prm = sfb.QPSolverParams(max_iter=max_iter)
    jobs = []
    for seed in seeds:
        P, q, A, l, u = _dense_data(sfb, n, m, B, seed, recipe)
        inputs = dict(P=P, q=q, A=A, l=l, u=u)
        wx = wy = None
        if warm:                 # tests/test_qp_dense_gpu.py::test_warm_start_batch
            ref0 = oracle.qp_dense_solve_batch(P, q, A, l, u, params=_oracle_params(oracle, prm), nthreads=8)
            wx = np.where(np.isfinite(ref0["x"]), ref0["x"], 0.0)
            wy = np.where(np.isfinite(ref0["y"]), ref0["y"], 0.0)
            inputs["q"] = q = q + 0.01
            inputs.update(warm_x=wx, warm_y=wy)
        outputs, inout, keep = _qp_outputs(B, n, m), {}, []
        if entry in ("trace", "phases"):
            inout["trace"] = np.full((B, rows, 5), -1.0)
        if entry == "phases":
            outputs["phase_us"] = ((B, 16), np.float64)
        ws = sfb.Workspace.for_dense(B, n, m, prm) if entry == "ws" else None
        keep.append(ws)

        def call(p, stream, ws=ws):
            a = (B, n, m, p["P"], p["q"], p["A"], p["l"], p["u"], p["x"], p["y"], p["obj"], p["iter"], p["code"])
            kw = dict(prm=prm, dwarm_x=p.get("warm_x", 0), dwarm_y=p.get("warm_y", 0), stream=stream)
            if entry == "ws":
                sfb.solve_qp_batch_device_ws(*a, ws, **kw)
            elif entry == "trace":
                sfb.solve_qp_batch_device_trace(*a, p["trace"], rows, **kw)
            elif entry == "phases":
                sfb.solve_qp_batch_device_phases(*a, p["phase_us"], dtrace=p["trace"], trace_rows=rows, **kw)
            elif entry == "tall":
                sfb.solve_qp_tall_batch_device(*a, **kw)
            else:
                sfb.solve_qp_batch_device(*a, **kw)

        def check(r, d=(P, q, A, l, u), wx=wx, wy=wy):
            ref = oracle.qp_dense_solve_batch(*d, params=_oracle_params(oracle, prm), nthreads=8, warm_x=wx, warm_y=wy,
                                              **({"trace_rows": rows} if "trace" in r else {}))
            if compare == "full_pattern":
                _compare_full_pattern(_qp_solution(sfb, r), ref, B)
            else:
                _compare(_qp_solution(sfb, r), ref)
            if "trace" in r:
                _compare_trace(r["trace"], ref["trace"], B)

        jobs.append(Job(inputs, inout, outputs, call, check, _drop_times if inout or "phase_us" in outputs else None, keep))
    return jobs


def tall_case(sfb, oracle, n, m, B):
    """the reduced-KKT route; reference: the oracle-free optimality certificates of tests/qp_certify.py on every item"""
    import qp_certify as QC
    import qp_families as QF
    cp = QC.Params(max_iter=4000)
    prm = cp.sfb(sfb)
    jobs = []
    for seed in (31 * n + m, 31 * n + m + 1):
        verdict, (P, q, A, l, u) = QF.build("pd_mixed", B, n, m, seed=seed)
        mm = l.shape[1]

        def call(p, stream, mm=mm):
            sfb.solve_qp_tall_batch_device(B, n, mm, p["P"], p["q"], p["A"], p["l"], p["u"], p["x"], p["y"], p["obj"], p["iter"], p["code"], prm=prm,
                                           stream=stream)

        def check(r, prob=QC.Problem.dense(P, q, A, l, u), verdict=verdict):
            rep = QC.certify(prob, _qp_solution(sfb, r), cp)
            assert rep.passed, str(rep)
            assert QF.verdict_ok(verdict, r["code"], cp, "pd_mixed").all(), r["code"]

        jobs.append(Job(dict(P=P, q=q, A=A, l=l, u=u), {}, _qp_outputs(B, n, mm), call, check))
    return jobs


_SPARSE = {}


def _sparse_problem(sfb, oracle, variant, K, B, seeds, pruned):
    """plan, data of both seeds and (lazily) the oracle's results: shared by the cases on the same problem"""
    key = (variant, K, B, seeds, pruned)
    if key not in _SPARSE:
        from examples import models_lib as M
        d, Pp, Pi, Pv, Ap, Aj = M.mpc_pattern(variant, K)
        data = [M.mpc_assemble_batch(variant, K, B, seed=s) for s in seeds]
        keep = np.any(np.concatenate([a[0] for a in data]) != 0.0, axis=0) if pruned else None
        plan = sfb.SparseQPPlan(d["n"], d["m"], Pp, Pi, Ap, Aj, stage=M.mpc_stage(variant, K), keep=keep)
        _SPARSE[key] = dict(d=d, pat=(Pp, Pi, Ap, Aj), Px=np.tile(Pv, (B, 1)), q=np.zeros((B, d["n"])), data=data, plan=plan, ref={})
    return _SPARSE[key]


def sparse_case(sfb, oracle, variant, K, B, entry="plain", seeds=(43, 44), pruned=False, prm=None, rows=12):
    import torch
    from test_qp_dense_gpu import _compare, _compare_trace, _oracle_params
    prm = sfb.QPSolverParams() if prm == "default" else (prm or sfb.QPSolverParams(max_iter=4000))
    S = _sparse_problem(sfb, oracle, variant, K, B, seeds, pruned)
    plan, (Pp, Pi, Ap, Aj), n, m = S["plan"], S["pat"], S["d"]["n"], S["d"]["m"]
    rng = np.random.default_rng(B)
    orders = [rng.permutation(B).astype(np.int32), np.arange(B, dtype=np.int32)[::-1].copy()]   # both valid permutations
    jobs = []
    for which, (Av, l, u) in enumerate(S["data"]):
        inputs = dict(Px=S["Px"], q=S["q"], Ax=Av, l=l, u=u)
        outputs, inout = _qp_outputs(B, n, m), {}
        if entry == "ordered":
            inputs["order"] = orders[which]
        if entry in ("trace", "phases"):
            inout["trace"] = np.full((B, rows, 5), -1.0)
        if entry == "phases":
            outputs["phase_us"] = ((B, 6), np.float64)
        ws = torch.empty(plan.workspace_bytes(B) + 16, dtype=torch.uint8, device="cuda:0")

        def call(p, stream, ws=ws):
            a = (B, p["Px"], p["q"], p["Ax"], p["l"], p["u"], p["x"], p["y"], p["obj"], p["iter"], p["code"], ws.data_ptr())
            if entry == "trace":
                plan.solve_batch_device_trace(*a, p["trace"], rows, prm, stream=stream)
            elif entry == "phases":
                plan.solve_batch_device_phases(*a, p["phase_us"], prm, stream=stream, dtrace=p["trace"], trace_rows=rows)
            else:
                plan.solve_batch_device(*a, prm, stream=stream, dorder=p.get("order", 0))

        def check(r, which=which, Av=Av, l=l, u=u):
            traced = "trace" in r
            if (which, traced, repr(prm)) not in S["ref"]:
                S["ref"][which, traced, repr(prm)] = oracle.qp_sparse_solve_batch(Pp, Pi, S["Px"], S["q"], Ap, Aj, Av, l, u, perm=plan.perm, forder=plan.factor_order(),
                                                                       params=_oracle_params(oracle, prm), nthreads=8, **({"trace_rows": rows} if traced else {}))
            ref = S["ref"][which, traced, repr(prm)]
            _compare(_qp_solution(sfb, r), ref)
            if traced:
                _compare_trace(r["trace"], ref["trace"], B)

        jobs.append(Job(inputs, inout, outputs, call, check, _drop_times if inout or "phase_us" in outputs else None, [plan, ws]))
    return jobs


def mpc_assemble_case(sfb, oracle, variant, K, B, shared):
    """reference: the host transcription (examples/models.cpp through the harness), bit for bit"""
    from examples import models_lib as M
    jobs = []
    for seed in (9, 10):
        want = M.mpc_assemble_batch(variant, K, B, seed=seed)
        L, rec = M.mpc_records(variant, K, B, seed=seed)
        inputs = dict(records=rec)
        if shared:
            own, sh = L.split_shared(rec)
            inputs = dict(records=np.ascontiguousarray(own), shared_jac=np.ascontiguousarray(sh))

        def call(p, stream, L=L):
            L.assemble_batch_device(B, p["records"], p["Ax"], p["l"], p["u"], p.get("shared_jac", 0), stream)

        def check(r, want=want):
            assert np.array_equal(r["Ax"], want[0]) and np.array_equal(r["l"], want[1]) and np.array_equal(r["u"], want[2])

        jobs.append(Job(inputs, {}, {"Ax": ((B, L.nnzA), np.float64), "l": ((B, L.m), np.float64), "u": ((B, L.m), np.float64)}, call, check, None, [L]))
    return jobs


def ekf_case(sfb, oracle, which, dof, ny, B):
    """reference: the 60-digit fixture within the gates of tests/ekf_gates.py; real: the draws of level c1, decoy: of level c6"""
    import ekf_gates as G
    jobs = []
    for L in ("c1", "c6"):
        s = G.state(dof, L)
        p = G.pair(dof, ny, L) if ny else {}
        a = {k: _tile(s[k], B) for k in ("A", "Q", "dt")}
        if which == "rk4_tv":
            a.update(Am=_tile(s["Am"], B), Ae=_tile(s["Ae"], B))
        upd = which in ("update", "fused")
        if upd:
            a.update({k: _tile(p[k], B) for k in ("H", "R", "r")})
        if which == "update":
            a = {k: a[k] for k in ("H", "R", "r")}
        outputs = {"delta": ((B, dof), np.float64), "info": ((B,), np.int32)} if upd else {}

        def call(q, stream):
            if which == "euler":
                sfb.ekf_predict_batch_device(B, dof, q["A"], q["Q"], 0, q["dt"], 0, q["P"], stream)
            elif which == "rk4":
                sfb.ekf_predict_stepper_batch_device("rk4", B, dof, q["A"], q["Q"], 0, q["dt"], 0, q["P"], stream)
            elif which == "rk4_tv":
                sfb.ekf_predict_rk4_batch_device(B, dof, q["A"], q["Am"], q["Ae"], q["Q"], 0, q["dt"], 0, q["P"], stream)
            elif which == "update":
                sfb.ekf_update_batch_device(B, dof, ny, q["H"], q["R"], 0, q["r"], q["P"], q["delta"], q["info"], stream)
            else:
                sfb.ekf_predict_update_batch_device(B, dof, ny, q["A"], q["Q"], 0, q["dt"], 0, q["H"], q["R"], 0, q["r"], q["P"], q["delta"], q["info"], stream)

        def check(r, L=L, s=s, p=p):
            if upd:
                cls = "update" if which == "update" else "fused"
                assert (r["info"] == 0).all()
                G.check(G.key(cls + "_P", dof, ny, L), r["P"], _tile(p[cls + "_P"], B), "stream contract")
                G.check(G.key(cls + "_delta", dof, ny, L), r["delta"], _tile(p[cls + "_delta"], B), "stream contract")
            else:
                G.check(G.key(which, dof, None, L), r["P"], _tile(s[which], B), "stream contract")

        jobs.append(Job(a, {"P": _tile(s["P"], B)}, outputs, call, check))
    return jobs


def pid_case(sfb, oracle, which, group, B):
    """reference: the 60-digit fixture within the gates of tests/pid_gates.py (sections step with windup 0.5, rollB)"""
    import pid_gates as G
    grp = sfb.PIDGroup(G.GROUPS[group])
    d = G.section("step" if which == "step" else "roll", group)
    real = {k: _tile(v, B) for k, v in d.items() if k != "umax"}
    jobs = []
    for a in (real, _rolled(real)):
        if which == "step":
            inputs = {k: a[k] for k in ("x", "v", "gd", "vd", "ad", "kp", "kd", "ki")}
            inout = {"ie": a["ie"], "t_last": a["t_last"]}
            outputs = {"u": ((B, grp.dof), np.float64)}

            def call(p, stream):
                sfb.pid_step_batch_device(grp, B, G.T_STEP, p["x"], p["v"], p["gd"], p["vd"], p["ad"], 0, p["kp"], p["kd"], p["ki"], 0, G.WINDUP, p["ie"],
                                          p["t_last"], p["u"], stream)

            def check(r, a=a):
                assert np.all(r["t_last"] == G.T_STEP)
                G.check("step", group, [("u", r["u"], a["u_w"]), ("ie", r["ie"], a["ie_w"])], a["cls"], "stream contract")
        else:
            steps = G.ROLL_SETS["B"][0]
            inputs = {k: a[k] for k in ("g0", "w", "kp", "kd", "ki")}
            inout = {"x": a["x"], "v": a["v"], "ie": a["ie"], "t_last": a["t_last"]}
            outputs = {"u_last": ((B, grp.dof), np.float64), "cost": ((B,), np.float64)}

            def call(p, stream):
                sfb.pid_rollout_batch_device(grp, B, G.T0, G.DT, steps, p["x"], p["v"], p["g0"], p["w"], 0, p["kp"], p["kd"], p["ki"], 0, G.WINDUP, 0, p["ie"],
                                             p["t_last"], p["u_last"], p["cost"], stream)

            def check(r, a=a):
                G.check("rollB", group, [("x", r["x"], a["x_B"]), ("v", r["v"], a["v_B"]), ("ie", r["ie"], a["ie_B"]), ("u", r["u_last"], a["u_B"]),
                                         ("cost", r["cost"], a["cost_B"])], a["cls"], "stream contract")
        jobs.append(Job(inputs, inout, outputs, call, check, None, [grp]))
    return jobs


# the 60-digit fixture of the five-knot SE3 curves (tests/golden/make_golden_spline5.py) and what the float64 restatement
# tests/spline_ref.py delivers against it per case class -- the gate rule of tests/spline_gates.py on these curves: a comparison's gate
# is MARGIN = 4 times this.  Measured by test_stream_contract_gpu.py::test_five_knot_gate_is_four_times_the_restatements_error on the CPU
# this was written on; neither a kernel nor the host front is its source.
SPLINE5_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spline5_reference.npz")
SPLINE5_MEASURED = {
    "fit.tiny": 2.64e-16, "fit.generic": 2.38e-16, "fit.abelian": 2.49e-16,
    "eval.tiny": 2.31e-16, "eval.generic": 4.80e-16, "eval.abelian": 3.12e-16,
    "rollB.tiny": 1.08e-15, "rollB.generic": 8.91e-16, "rollB.abelian": 6.16e-16,
}
_SPLINE5 = {}


def _five_knot_curves(group="SE3"):
    """the fixture's four-knot curves (S = 3) with a fifth knot, the last increment once more: g_4 = g_3 (+) (g_3 (-) g_2) at
    t_4 = t_3 + (t_3 - t_2), so every curve keeps its knot class; inputs and 60-digit results (V, g, vel, acc, rollouts)"""
    assert group == "SE3"
    if group not in _SPLINE5:
        _SPLINE5[group] = dict(np.load(SPLINE5_FIXTURE))
    return _SPLINE5[group]


def spline5_restatement_errors(group="SE3"):
    """{"section.class": error of tests/spline_ref.py against the five-knot fixture}"""
    import spline_gates as G
    import spline_ref as SR
    d, parts = _five_knot_curves(group), G.GROUPS[group]
    steps = G.ROLL_SETS["B"][0]
    r = SR.rollout(parts, G.T0, G.DT, steps, d["x"], d["v"], d["tk"], d["gk"], d["V"], d["ts0"], d["kp"], d["kd"], d["ki"], G.WINDUP, None, d["t_last"], d["ie"])
    pairs = {"fit": [("V", SR.fit(parts, d["tk"], d["gk"]), d["V"])],
             "eval": G.eval_pairs(d, SR.evaluate(parts, d["tk"], d["gk"], d["V"], d["t"])),
             "rollB": [(k, r[k], d["%s_B" % k]) for k in ("x", "v", "ie", "u", "cost")]}
    return {"%s.%s" % (sec, c): e for sec, pp in pairs.items() for c, e in G.errors(group, pp, d["cls"]).items()}


def _spline_check(sec, group, pairs, cls):
    """kernel against the 60-digit five-knot fixture, per class within 4 x SPLINE5_MEASURED; the figures are printed first"""
    import spline_gates as G
    err = G.errors(group, pairs, cls)
    gate = {c: G.MARGIN * SPLINE5_MEASURED["%s.%s" % (sec, c)] for c in err}
    print("%-7s %-6s stream contract, 5 knots   %s" % (sec, group, "  ".join("%s %.2e (gate %.2e)" % (c, e, gate[c]) for c, e in sorted(err.items()))))
    bad = {c: (e, gate[c]) for c, e in err.items() if not e <= gate[c]}
    assert not bad, "%s %s, 5 knots: over the gate: %s" % (sec, group, bad)


def spline_case(sfb, oracle, which, group, B):
    import spline_gates as G
    grp = sfb.PIDGroup(G.GROUPS[group])
    d = _five_knot_curves(group)
    real = {k: _tile(v, B) for k, v in d.items() if k != "umax"}
    K = real["tk"].shape[1]
    nt = real["t"].shape[1]
    jobs = []
    for a in (real, _rolled(real)):
        if which == "fit":
            inputs, inout, outputs = {k: a[k] for k in ("tk", "gk")}, {}, {"V": ((B, K - 1, 3, grp.dof), np.float64)}

            def call(p, stream):
                sfb.spline_fit_cubic_batch_device(grp, B, K, p["tk"], 0, p["gk"], p["V"], stream)

            def check(r, a=a):
                _spline_check("fit", group, [("V", r["V"], a["V"])], a["cls"])
        elif which == "eval":
            inputs, inout = {k: a[k] for k in ("tk", "gk", "V", "t")}, {}
            outputs = {"g": ((B, nt, grp.elem), np.float64), "vel": ((B, nt, grp.dof), np.float64), "acc": ((B, nt, grp.dof), np.float64)}

            def call(p, stream):
                sfb.spline_eval_batch_device(grp, B, K, p["tk"], p["gk"], p["V"], 0, 0, nt, p["t"], 0, p["g"], p["vel"], p["acc"], stream)

            def check(r, a=a):
                _spline_check("eval", group, [("g", r["g"], a["g"]), ("vel", r["vel"], a["vel"]), ("acc", r["acc"], a["acc"])], a["cls"])
        else:
            steps = G.ROLL_SETS["B"][0]
            inputs = {k: a[k] for k in ("tk", "gk", "V", "ts0", "kp", "kd", "ki")}
            inout = {"x": a["x"], "v": a["v"], "ie": a["ie"], "t_last": a["t_last"]}
            outputs = {"u_last": ((B, grp.dof), np.float64), "cost": ((B,), np.float64)}

            def call(p, stream):
                sfb.pid_rollout_spline_batch_device(grp, B, G.T0, G.DT, steps, p["x"], p["v"], K, p["tk"], p["gk"], p["V"], 0, p["ts0"], p["kp"], p["kd"], p["ki"], 0,
                                                    G.WINDUP, 0, p["ie"], p["t_last"], p["u_last"], p["cost"], stream)

            def check(r, a=a):
                _spline_check("rollB", group, [("x", r["x"], a["x_B"]), ("v", r["v"], a["v_B"]), ("ie", r["ie"], a["ie_B"]), ("u", r["u_last"], a["u_B"]),
                                               ("cost", r["cost"], a["cost_B"])], a["cls"])
        jobs.append(Job(inputs, inout, outputs, call, check, None, [grp]))
    return jobs


def mesh_case(sfb, oracle, which, B):
    """reference: the 60-digit fixture within the gates of tests/mesh_gates.py, on the smallest mesh of the entry's own test;
    every agent carries the fixture's values, the decoy a scaled and shifted copy"""
    import mesh_gates as G
    if which == "resample":
        name = min(G.MESHES, key=lambda n: int(np.sum(G.mesh(n)["K"])))
        m, r = G.mesh(name), G.section("resample." + name)
        mesh = sfb.PHMesh(m["K"], m["tau0"])
        vals = np.ascontiguousarray(np.broadcast_to(r["vals"], (B,) + r["vals"].shape))
        dim = vals.shape[2]

        def call(p, stream):
            sfb.mesh_resample_batch_device(mesh, B, dim, True, p["vals"], p["out"], stream)

        def check(res):
            for b in sorted({0, B // 2, B - 1}):
                G.check("resample", res["out"][b], r["out_ext"], "%s agent %d, stream contract" % (name, b))

        return [Job({"vals": v}, {}, {"out": ((B, mesh.R, dim), np.float64)}, call, c, None, [mesh]) for v, c in ((vals, check), (1.5 * vals + 0.25, None))]
    from test_mesh_gpu import _samples
    name = min(G.DYN, key=lambda n: int(np.sum(G.dyn(n)["base"]["K"])) * int(G.dyn(n)["nx"]))
    d, X, U, F = _samples(name)
    mesh = sfb.PHMesh(d["base"]["K"], d["base"]["tau0"])
    nx = int(d["nx"])
    tile = lambda a: np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))       # noqa: E731
    h = np.full(B, float(d["tf"]) - float(d["t0"]))

    def call(p, stream):
        sfb.mesh_dyn_error_batch_device(mesh, B, nx, p["horizon"], p["X"], p["F"], p["errs"], stream)

    def check(res):
        for b in sorted({0, B // 2, B - 1}):
            G.check("dynerr." + d["cls_name"], res["errs"][b], d["errs"], "%s agent %d, stream contract" % (name, b))

    out = {"errs": ((B, mesh.nivals), np.float64)}
    return [Job(dict(horizon=h, X=tile(X), F=tile(F)), {}, out, call, check, None, [mesh]),
            Job(dict(horizon=1.25 * h, X=1.5 * tile(X) + 0.25, F=0.75 * tile(F)), {}, out, call, None, None, [mesh])]


def meshfn_case(sfb, oracle, key, B):
    """reference: the 60-digit fixture (even agents) and the host front (odd agents) within the gates of tests/meshfn_gates.py, as in
    tests/test_meshfn_gpu.py, on its smallest case that has the function"""
    import meshfn_gates as G
    from test_meshfn_gpu import _batch, _dims, _draws
    names = [n for n in G.CASES if str(G.case(n)["fn"]) != "vehicle" and key + ".F" in G.case(n)]
    name = min(names, key=lambda n: int(np.sum(G.case(n)["m"]["K"])) * max(1, _dims(G.case(n))[0]))
    c, draws = _draws(name)
    nx, nu, nf = _dims(c)
    mesh = sfb.PHMesh(c["m"]["K"], c["m"]["tau0"])
    which, t0, tf, X, F, dF = _batch(draws, B, False)
    real = dict(t0=t0, tf=tf, F=F, dF=dF)
    if key == "dyn":
        real["X"] = X
    N = mesh.N
    if key == "integrate":
        outputs = {"out_F": ((B, nf), np.float64), "out_dF": ((B, nf, 2 + nx * (N + 1) + nu * N), np.float64)}
    elif key == "dyn":
        outputs = {"out_F": ((B, N * nx), np.float64), "out_dF": ((B, len(sfb.mesh_dyn_pattern(mesh, nx, nu)[1])), np.float64)}
    else:
        outputs = {"out_F": ((B, N * nf), np.float64), "out_dF": ((B, N * nf * (2 + nx + nu)), np.float64)}

    def call(p, stream):
        if key == "dyn":
            sfb.mesh_dyn_batch_device(mesh, B, nx, nu, p["t0"], p["tf"], p["X"], p["F"], p["dF"], p["out_F"], p["out_dF"], stream)
        elif key == "integrate":
            sfb.mesh_integrate_batch_device(mesh, B, nx, nu, nf, p["t0"], p["tf"], p["F"], p["dF"], p["out_F"], p["out_dF"], stream)
        else:
            sfb.mesh_eval_batch_device(mesh, B, nx, nu, nf, key == "evals", p["t0"], p["tf"], p["F"], p["dF"], p["out_F"], p["out_dF"], stream)

    def check(r):
        for b in sorted({0, 1, 2, B // 2, B - 2, B - 1} & set(range(B))):
            ref = c if which[b] == 0 else draws[which[b]]
            who = "%s agent %d %s, stream contract" % (name, b, "fixture" if which[b] == 0 else "host front")
            G.check(key + ".F", r["out_F"][b].ravel(), ref[key + ".F"], who)
            G.check(key + ".dF", r["out_dF"][b].ravel(), ref[key + ".dF"], who)

    return [Job(real, {}, outputs, call, check, None, [mesh]), Job(_rolled(real), {}, outputs, call, None, None, [mesh])]


def ocpnlp_case(sfb, oracle, hess, B):
    """reference: the 60-digit fixture (even agents) and the host front (odd agents) within the gates of tests/ocpnlp_gates.py /
    ocpnlp_hess_gates.py, as in tests/test_ocpnlp_gpu.py / test_ocpnlp_hess_gpu.py, on the smallest case"""
    import ocpnlp_gates as G
    import ocpnlp_hess_gates as HG
    import test_ocpnlp_gpu as T1
    import test_ocpnlp_hess_gpu as T2
    name = min(G.CASES, key=lambda n: len(G.case(n)["dg"]) + len(G.case(n)["g"]))
    T = T2 if hess else T1
    c, draws = T._draws(name)
    mesh = sfb.PHMesh(c["m"]["K"], c["m"]["tau0"])
    dims = [int(v) for v in c["dims"]]
    which, a = T._batch(draws, B)
    real = {k: np.ascontiguousarray(np.asarray(v, dtype=np.float64)) for k, v in a.items()}
    if hess:
        outputs = {"hess": ((B, len(c["h.rowind"])), np.float64)}

        def call(p, stream):
            sfb.ocp_nlp_hess_batch_device(mesh, dims, B, *[p[k] for k in T2.NAMES], p["hess"], stream)

        def check(r):
            for b in range(B):
                HG.check(r["hess"][b], draws[which[b]]["ref"], "%s agent %d, stream contract" % (name, b))
    else:
        outputs = {"g": ((B, len(c["g"])), np.float64), "dg": ((B, len(c["dg"])), np.float64)}

        def call(p, stream):
            sfb.ocp_nlp_batch_device(mesh, dims, B, p["x"], *[p[k] for k in T1.NAMES], p["g"], p["dg"], stream)

        def check(r):
            for b in range(B):
                G.check("g", r["g"][b], draws[which[b]]["g"], "%s agent %d, stream contract" % (name, b))
                G.check("dg", r["dg"][b], draws[which[b]]["dg"], "%s agent %d, stream contract" % (name, b))

    return [Job(real, {}, outputs, call, check, None, [mesh]), Job(_rolled(real), {}, outputs, call, None, None, [mesh])]


# ------------------------------------------------------------------------------------------------ the case table
@dataclass
class Case:
    entry: str                     # the function of sfb.h the case calls
    build: Callable                # (sfb, oracle) -> (real Job, decoy Job)
    knobs: dict = field(default_factory=dict)


def _c(c_name, fn, /, *args, knobs=None, **kw):
    return Case(c_name, lambda sfb, oracle: fn(sfb, oracle, *args, **kw), knobs or {})


D, S, E = "sfb_qp_dense_solve_batch", "sfb_sparse_qp_solve_batch", "sfb_ekf_"
HEADLINE = dict(seeds=(43, 44), pruned=True, prm="default")
CASES = {
    # dense, one case per route
    "dense four-per-wave k<=16 (3,5) B=41": _c(D, dense_case, 3, 5, 41),
    "dense four-per-wave k<=32 (10,20) B=65": _c(D, dense_case, 10, 20, 65),
    "dense four-per-wave (10,20) B=65, 3 waves (refill queue)": _c(D, dense_case, 10, 20, 65, knobs={"SFB_QP4_MAX_WAVES": 3}),
    "dense four-per-wave (10,20) B=65 warm start": _c(D, dense_case, 10, 20, 65, warm=True),
    "dense registers (20,30) B=25": _c(D, dense_case, 20, 30, 25),
    "dense LDS blocks (40,60) B=13": _c(D, dense_case, 40, 60, 13),
    "dense factor in HBM (3,203) B=6": _c(D, dense_case, 3, 203, 6, recipe="big", seeds=(203, 204)),
    # SFB_QP_DENSE_BIG=0 acts above n + m = 128 only (dense_solve_impl, csrc/capi.hip): (40,30) stays on the on-chip kernel of (40,60) and
    # is compared like it; (40,110), with the bands of a safety filter so that the items are feasible, takes dense_via_sparse (per-call memory, the A-by-rows kernel, the nested sparse solve)
    "dense (40,30) B=8, SFB_QP_DENSE_BIG=0 (still the on-chip kernel)": _c(D, dense_case, 40, 30, 8, recipe=0.6, seeds=(240, 241), knobs={"SFB_QP_DENSE_BIG": 0}),
    "dense full-pattern sparse route (40,110) B=8": _c(D, dense_case, 40, 110, 8, recipe="big", seeds=(240, 241), compare="full_pattern",
                                                       knobs={"SFB_QP_DENSE_BIG": 0}),
    "dense_ws (10,20) B=65": _c(D + "_ws", dense_case, 10, 20, 65, entry="ws"),
    "dense_ws (3,203) B=6": _c(D + "_ws", dense_case, 3, 203, 6, entry="ws", recipe="big", seeds=(203, 204)),
    "dense_trace (10,20) B=8": _c(D + "_trace", dense_case, 10, 20, 8, entry="trace", recipe=0.9, max_iter=202, seeds=(23, 24)),
    "dense_phases (10,20) B=8": _c(D + "_phases", dense_case, 10, 20, 8, entry="phases", recipe=0.9, max_iter=202, seeds=(23, 24)),
    "dense_tall in LDS (3,203) B=8": _c("sfb_qp_dense_tall_solve_batch", tall_case, 3, 203, 8),
    "dense_tall beyond LDS (8,800) B=4": _c("sfb_qp_dense_tall_solve_batch", tall_case, 8, 800, 4),
    # sparse
    "sparse MPC variant 6 K=10 B=7": _c(S, sparse_case, 6, 10, 7),
    "sparse headline variant 12 K=50 B=72, grid 12": _c(S, sparse_case, 12, 50, 72, **HEADLINE, knobs={"SFB_SP_GRID": 12}),
    "sparse headline B=72, grid 12, no polishers": _c(S, sparse_case, 12, 50, 72, **HEADLINE, knobs={"SFB_SP_GRID": 12, "SFB_SP_POLISHERS": 0}),
    "sparse_ordered variant 6 K=10 B=7": _c(S + "_ordered", sparse_case, 6, 10, 7, entry="ordered"),
    "sparse_trace variant 6 K=10 B=7": _c(S + "_trace", sparse_case, 6, 10, 7, entry="trace"),
    "sparse_phases variant 6 K=10 B=7": _c(S + "_phases", sparse_case, 6, 10, 7, entry="phases"),
    "mpc_assemble (6,10) B=7": _c("sfb_mpc_assemble_batch", mpc_assemble_case, 6, 10, 7, False),
    "mpc_assemble (6,10) B=7 shared_jac": _c("sfb_mpc_assemble_batch", mpc_assemble_case, 6, 10, 7, True),
    # EKF
    "ekf_predict dof 6 B=130": _c(E + "predict_batch", ekf_case, "euler", 6, 0, 130),
    "ekf_update (6,3) B=130": _c(E + "update_batch", ekf_case, "update", 6, 3, 130),
    "ekf_predict_update (6,3) B=130": _c(E + "predict_update_batch", ekf_case, "fused", 6, 3, 130),
    "ekf_predict_update wide (10,3) B=130": _c(E + "predict_update_batch", ekf_case, "fused", 10, 3, 130),
    "ekf_predict_stepper rk4 dof 6 B=130": _c(E + "predict_stepper_batch", ekf_case, "rk4", 6, 0, 130),
    "ekf_predict_rk4 A_mid A_end dof 6 B=130": _c(E + "predict_rk4_batch", ekf_case, "rk4_tv", 6, 0, 130),
    # PID and splines
    "pid_step SE3 B=65": _c("sfb_pid_step_batch", pid_case, "step", "SE3", 65),
    "pid_rollout SE3 B=65": _c("sfb_pid_rollout_batch", pid_case, "roll", "SE3", 65),
    "spline_fit_cubic SE3 5 knots B=65": _c("sfb_spline_fit_cubic_batch", spline_case, "fit", "SE3", 65),
    "spline_eval SE3 5 knots B=65": _c("sfb_spline_eval_batch", spline_case, "eval", "SE3", 65),
    "pid_rollout_spline SE3 5 knots B=65": _c("sfb_pid_rollout_spline_batch", spline_case, "roll", "SE3", 65),
    # meshes and the collocation NLP
    "mesh_resample B=65": _c("sfb_mesh_resample_batch", mesh_case, "resample", 65),
    "mesh_dyn_error B=65": _c("sfb_mesh_dyn_error_batch", mesh_case, "dyn_error", 65),
    "mesh_eval B=65": _c("sfb_mesh_eval_batch", meshfn_case, "eval", 65),
    "mesh_integrate B=65": _c("sfb_mesh_integrate_batch", meshfn_case, "integrate", 65),
    "mesh_dyn B=65": _c("sfb_mesh_dyn_batch", meshfn_case, "dyn", 65),
    "ocp_nlp B=5": _c("sfb_ocp_nlp_batch", ocpnlp_case, False, 5),
    "ocp_nlp_hess B=5": _c("sfb_ocp_nlp_hess_batch", ocpnlp_case, True, 5),
}
