"""Which library calls does the engine make, with which arguments?  (Needs a GPU; seconds per case.)

    python scripts/trace_launches.py [--dry] OUT.jsonl [CASE ...]

What a change of the engine's HOST code has to show (NOTEBOOK R10.1): run this on the parent and on the change and `diff` the two files.
Every callable export of the loaded library object is wrapped (tests/test_epilogue_plain.py's `launches` fixture does it for three).  One
engine per entry of tests/test_nonfinite.py's MATRIX -- every route of the library at the smallest shapes that still have a ragged last
tile, padded slots or several blocks -- plus chunked shards (plain, deterministic, a chain with a lane block, a frozen scaler), the three class flags flipped, an explicit
reflection-owner shard and shards of harmonic groups.  Each engine runs two `train_step` calls and one `evaluate_nll` on a `make_obs`
set with in-kernel noise, then the same with injected `u_f` / `eta` and a `forward_backward` with `ipred_out`.  Behind them the
forward-only scaler path (`engine.scaler_forward`) on each of its routes: the cases of tests/test_scaler_forward.py, one
`model.scaling_model(inputs)` and one `model.scale_mean_stddev(inputs)` each, the unbalanced-image case a second time in row chunks of 128.

One line per call: the entry point, its return value, every scalar argument, every non-pointer struct field, and for every pointer null,
"outside" (a flag of a query, a host buffer) or [byte size of the live device storage that holds it, offset into it] -- the storages are
looked up among the live CUDA tensors, so the record depends neither on attribute names nor on the allocator's addresses.

`--dry` needs no GPU: the engine builds its buffers in host memory, every entry point that takes a stream is recorded and NOT called
(it "returns" 0), the host queries (routes, sizes, names) are.  The host code makes no decision from a kernel's result, so the record
is the one a device run gives, up to the answers of the two fused wide launches that may decline a shape (-2 on a device, 0 here).
"""
from __future__ import annotations

import bisect
import ctypes as C
import gc
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from careless_amd import _lib  # noqa: E402


class Tracer:
    def __init__(self, out, dry=False):
        self.out, self.starts, self.size, self.dry = out, [], {}, dry
        lib = _lib.get_lib()
        for name, (res, argtypes) in _lib.EXPORTS.items():
            launch = bool(argtypes) and argtypes[-1] is C.c_void_p and res is C.c_int and not name.startswith("cl_host_")      # (its last argument is the stream)
            setattr(lib, name, self._wrap(name, getattr(lib, name), res, argtypes, dry and launch))
        if dry:
            import careless_amd.engine  # noqa: F401      (the stubs go on every loaded module of the package that holds the name)
            stubs = dict(require_gpu=lambda what: torch.device("cpu"), _stream=lambda: 0)
            for mod in [m for n, m in list(sys.modules.items()) if n.startswith("careless_amd.") and m is not None]:
                for name, stub in stubs.items():
                    if hasattr(mod, name):
                        setattr(mod, name, stub)
            torch.cuda.synchronize = lambda *a: None
            torch.cuda.mem_get_info = lambda *a: (64 << 30, 64 << 30)

    def rescan(self):
        """The live device storages: start -> bytes."""
        self.size = {}
        for o in gc.get_objects():
            try:
                if isinstance(o, torch.Tensor) and (o.is_cuda or self.dry):
                    s = o.untyped_storage()
                    if s.data_ptr():
                        self.size[s.data_ptr()] = max(self.size.get(s.data_ptr(), 0), s.nbytes())
            except Exception:               # (objects that do not survive an isinstance question)
                pass
        self.starts = sorted(self.size)

    def _find(self, p):
        k = bisect.bisect_right(self.starts, p) - 1
        if k >= 0 and p <= self.starts[k] + self.size[self.starts[k]]:          # (the end of a buffer: an empty slice behind its last part)
            return [self.size[self.starts[k]], p - self.starts[k]]
        return None

    def pointer(self, p):
        if not p:
            return None
        if p < 4096:                        # (a query's "this buffer is given" flag)
            return "outside"
        hit = self._find(p)
        if hit is None:                     # a buffer born since the last look
            self.rescan()
            hit = self._find(p)
        return hit if hit is not None else "outside"

    def value(self, v, ctype):
        if ctype is C.c_void_p:
            return self.pointer(v)
        if isinstance(ctype, type) and issubclass(ctype, C.Array):
            return list(v)
        return v

    def _wrap(self, name, fn, res, argtypes, skip):
        def wrapped(*args):
            rec = []
            if self.dry:                    # (host memory is handed out again at once: look at what lives now)
                self.rescan()
            for a, t in zip(args, argtypes):
                if isinstance(t, type) and issubclass(t, C._Pointer) and issubclass(t._type_, C.Structure):
                    s = a._obj if hasattr(a, "_obj") else a
                    rec.append(None if s is None else {f: self.value(getattr(s, f), ft) for f, ft in s._fields_})
                elif t is C.c_void_p:
                    rec.append(self.pointer(a if a is None or isinstance(a, int) else C.cast(a, C.c_void_p).value))
                elif t in (C.c_char_p,) or (isinstance(t, type) and issubclass(t, C._Pointer)):
                    rec.append("host")
                else:
                    rec.append(a)
            ret = 0 if skip else fn(*args)
            self.out.write(json.dumps({"fn": name, "ret": ret.decode() if isinstance(ret, bytes) else ret, "args": rec}) + "\n")
            return ret
        return wrapped

    def mark(self, text):
        self.out.write("# " + text + "\n")
        self.out.flush()
        self.rescan()


def _problem(case):
    """The finite twin of tests/test_nonfinite.py's `_problem`."""
    from tests import test_gpu_parity as P
    from tests import util
    kw = dict(case.kw, seed=case.seed)
    opts = {k: kw.pop(k, None) for k in ("two_pass", "regroup", "shuffle_rows", "grid")}
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    if opts["regroup"]:
        data = P._regroup_laue(data, opts["regroup"])
    return kw, opts, dict(data), cfg, params, u_f, eta


def _phase(tr, what, fn):
    tr.mark(what)
    try:
        fn()
    except (NotImplementedError, ValueError) as e:          # (a call the engine refuses: the refusal is part of the record)
        tr.out.write(json.dumps({"raised": type(e).__name__, "msg": str(e)}) + "\n")
    torch.cuda.synchronize()


def run_engine(tr, name, eng, inputs, u_f, eta, injected=True):
    """Two steps and a validation pass with in-kernel noise, then with injected noise, then the call that asks for predictions."""
    eng.alloc_history(4)
    _phase(tr, f"{name}: train_step 0, in-kernel noise", lambda: eng.train_step(0))
    _phase(tr, f"{name}: train_step 1, in-kernel noise", lambda: eng.train_step(1))
    val = []
    _phase(tr, f"{name}: make_obs", lambda: val.append(eng.make_obs(inputs)))
    if val:
        _phase(tr, f"{name}: evaluate_nll, in-kernel noise", lambda: eng.evaluate_nll(val[0], 0x40000002))
    if not injected:
        return
    du, de = eng._noise_to_device(u_f, eta)
    _phase(tr, f"{name}: train_step 2, injected noise", lambda: eng.train_step(2, du, de))
    _phase(tr, f"{name}: train_step 3, injected noise", lambda: eng.train_step(3, du, de))
    if val:
        _phase(tr, f"{name}: evaluate_nll, injected noise", lambda: eng.evaluate_nll(val[0], 0x40000004, u_f, eta))
    ipred = torch.empty(eng.obs.N * eng.S, dtype=torch.float32, device=eng.device)
    _phase(tr, f"{name}: forward_backward, injected noise and ipred_out", lambda: eng.forward_backward(eng.t, du, de, ipred_out=ipred))


def matrix_case(tr, name, flags=None, cls_flags=None):
    from careless_amd.engine import ElboEngine
    from tests import test_nonfinite as NF
    from tests import util
    case = NF.MATRIX[name]
    kw, opts, data, cfg, params, u_f, eta = _problem(case)
    old = {k: getattr(ElboEngine, k) for k in (cls_flags or {})}
    try:
        for k, v in (cls_flags or {}).items():
            setattr(ElboEngine, k, v)
        tag = name + "".join(f" {k}={v}" for k, v in {**(cls_flags or {}), **(flags or {})}.items())
        tr.mark(f"{tag}: engine")
        inputs = util.reference_inputs(data)
        eng = NF._model(case, kw, opts, data, cfg, params).engine(inputs)
        for k, v in (flags or {}).items():
            setattr(eng, k, v)
        if not eng.wide and not case.frozen:
            eng.kernel_name()
        run_engine(tr, tag, eng, inputs, u_f, eta)
    finally:
        for k, v in old.items():
            setattr(ElboEngine, k, v)


def shard_case(tr, name, kw, shard_of, det=False, frozen=False, injected=True, env=None):
    """An engine on an explicit shard (`shard_of(data, kw)`), all-reduce skipped (`local_only`)."""
    from careless_amd.engine import ElboEngine
    from tests import util
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    model = util.build_model(data, cfg, params, kw["L"], kw["w"])
    model.deterministic = det
    if frozen:
        model.scaling_model.trainable = False
        model.frozen_scaler_fast_path = True
    inputs = util.reference_inputs(data)
    for k, v in (env or {}).items():
        os.environ[k] = v
    try:
        tr.mark(f"{name}: engine")
        eng = ElboEngine(model, inputs, seed=99, shard=shard_of(data, kw))
        eng.local_only = True
        run_engine(tr, name, eng, inputs, u_f, eta, injected=injected)
    finally:
        for k in (env or {}):
            del os.environ[k]


def forward_case(tr, name, budget=None):
    """The forward-only scaler path on a case of tests/test_scaler_forward.py (`budget`: `engine.FORWARD_CHUNK_BYTES` for the run)."""
    from careless_amd import engine
    from tests import test_scaler_forward as SF
    model, inputs = SF.build(name[len("forward_"):].replace("_chunk128", ""))[:2]
    old = engine.FORWARD_CHUNK_BYTES
    try:
        if budget is not None:
            engine.FORWARD_CHUNK_BYTES = budget
        _phase(tr, f"{name}: scaling_model(inputs)", lambda: model.scaling_model(inputs))
        _phase(tr, f"{name}: scale_mean_stddev(inputs)", lambda: model.scale_mean_stddev(inputs))
    finally:
        engine.FORWARD_CHUNK_BYTES = old


def extra_cases():
    from careless_amd.engine import make_shard, owner_shard
    from tests import test_frozen_scaler as F
    from tests import test_gpu_parity as P
    mono, laue = P.CASES["mlp2x32_normal_img_S3"], F.CASES["laue_2x32_S2"]
    rows128 = lambda kw, det: {"CARELESS_HIP_MAX_LAUNCH_BYTES": str(128 * 4 * max((kw["d0"] + 3) // 4 * 4, kw["S"] if det else 0))}
    out = {}
    for det in (False, True):           # 300 rows in launches of 128: three pieces
        out[f"chunked_mono_2x32{'_det' if det else ''}"] = lambda tr, n, det=det: shard_case(tr, n, mono, lambda d, kw: None, det=det, env=rows128(mono, det))
    deep = dict(N=300, R=30, d0=5, L=24, w=10, S=1, perturb=0.02)          # (tests/test_routing.py: the last 20 layers on the lane kernel, dZ_0 out)
    out["chunked_chain_lane_24x10"] = lambda tr, n: shard_case(tr, n, deep, lambda d, kw: None, env=rows128(deep, False))
    out["chunked_frozen_mono_2x32"] = lambda tr, n: shard_case(tr, n, mono, lambda d, kw: None, frozen=True, env=rows128(mono, False))
    out["frozen_mono_slot_rows"] = lambda tr, n: matrix_case(tr, "frozen_mono_20x10", flags=dict(FROZEN_SORTED_ROWS=False))
    out["frozen_laue_slot_launches"] = lambda tr, n: matrix_case(tr, "frozen_laue_two_call_form_2x32", cls_flags=dict(FROZEN_LAUE_PACKED=False))
    out["wide_three_slot_launches"] = lambda tr, n: matrix_case(tr, "wide_3x96", flags=dict(SLOT_ROWS_ONE_LAUNCH=False))
    out["owner_shard_mono_2x32"] = lambda tr, n: shard_case(tr, n, mono, lambda d, kw: owner_shard(np.asarray(d["refl_id"]), kw["R"], 1, 2))
    out["laue_group_shard_2x32"] = lambda tr, n: shard_case(tr, n, laue, lambda d, kw: make_shard(kw["N"], kw["R"], 1, 2))
    out["laue_group_shard_2x32_frozen"] = lambda tr, n: shard_case(tr, n, laue, lambda d, kw: make_shard(kw["N"], kw["R"], 1, 2), frozen=True,
                                                                    injected=False)
    from tests import test_scaler_forward as SF
    for name in SF.CASES:
        out["forward_" + name] = forward_case
    out[f"forward_{SF.UNBALANCED}_chunk128"] = lambda tr, n: forward_case(tr, n, SF.CHUNK_128)
    return out


def main(argv):
    dry = "--dry" in argv
    argv = [a for a in argv if a != "--dry"]
    if len(argv) < 2:
        print(__doc__)
        return 2
    from tests import test_nonfinite as NF
    extras = extra_cases()
    names = argv[2:] or list(NF.MATRIX) + list(extras)
    with open(argv[1], "w") as out:
        tr = Tracer(out, dry)
        for n in names:
            extras[n](tr, n) if n in extras else matrix_case(tr, n)
            gc.collect()
            print("traced", n, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
