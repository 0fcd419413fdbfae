"""What FusedSGDClip / FusedAdamWClip hand to the library, call by call, for every legal option combination.

Each case runs one short script through the optimizers' public methods with the library call wrapped by a recorder (as
test_eval_is_the_dropout_free_module_bit_for_bit in test_gpu_lora_dropout.py wraps `ops.call`) and compares the recorded
trace with tests/golden/optim_call_trace.json.  A trace entry is the entry-point name and its arguments: scalars as they
are, a pointer as the [role, parameter index] of the tensor it points to, and a descriptor table or a side table read back
from the device and decoded row by row the same way.

The golden file was written by this same file in record mode (LCV_RECORD_OPTIM_TRACE=1) on the commit before the
optimizers moved from lcv_hip/ops.py into lcv_hip/optim.py, with FusedSGDClip still carrying its own constructor and step()
and the four tables still built by hand; the recorder finds `call` in whichever of the two modules binds it, so the file runs
on both trees.  It is the record of what those classes passed, and a host-side rewrite of them must reproduce it exactly."""
import ctypes
import json
import os
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "optim_call_trace.json"
RECORD = os.environ.get("LCV_RECORD_OPTIM_TRACE", "") == "1"
DEV = "cuda"

# one chunk, the chunk boundary (FusedAdamWClip.CHUNK = 2048), a tensor that never gets a gradient, one element past the
# boundary, and a zero-element tensor without a gradient (the drift and the average tables skip it)
NUMELS = (1, 2048, 3, 2049, 0)
WITH_GRAD = (0, 1, 3)

# entry points whose first argument is a descriptor table: how many side tables (n_tensors pointers each) follow it, in
# front of n_tensors and total_chunks (the headers under include/)
SIDE_TABLES = {
    "lcv_grad_norm_clip": 0, "lcv_det_grad_norm_clip": 0, "lcv_adamw_step": 0, "lcv_sgd_step": 0,
    "lcv_master_sgd_step": 1, "lcv_master_adamw_step": 1, "lcv_master_sgd_step_g32": 1, "lcv_master_adamw_step_g32": 1,
    "lcv_grad_accumulate": 1,
    "lcv_master_sgd_step_anchor": 2, "lcv_master_adamw_step_anchor": 2, "lcv_master_adamw8_step": 2,
    "lcv_master_ema_load": 2, "lcv_master_ema_update": 2, "lcv_master_ema_swap": 2, "lcv_master_drift_sumsq": 2,
    "lcv_master_adamw8_step_anchor": 3,
}

FORMS = {   # master_weights, moments_8bit, grad_accum, anchor, fp32 parameters
    "bf16": (False, False, 1, False, False),
    "f32": (False, False, 1, False, True),
    "master": (True, False, 1, False, False),
    "master+accum": (True, False, 2, False, False),
    "master+anchor": (True, False, 1, True, False),
    "master+anchor+accum": (True, False, 2, True, False),
    "master+8bit": (True, True, 1, False, False),
    "master+8bit+anchor": (True, True, 1, True, False),
}


def _cases():
    for kind in ("sgd", "adamw"):
        for form, (master, m8, _, _, _) in FORMS.items():
            if m8 and kind == "sgd":
                continue
            for ema in ((False, True) if master else (False,)):
                for det in (False, True):
                    yield f"{kind}-{form}-{'ema' if ema else 'noema'}-{'det' if det else 'atomic'}"


def _read_i64(ptr: int, n: int):
    """n int64 words of device memory, through the HIP runtime the library itself is linked to."""
    from lcv_hip import lib
    torch.cuda.synchronize()
    host = (ctypes.c_int64 * n)()
    memcpy = lib.load().hipMemcpy
    memcpy.restype = ctypes.c_int
    memcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert memcpy(host, ptr, 8 * n, 2) == 0       # hipMemcpyDeviceToHost
    return list(host)


class _Recorder:
    def __init__(self):
        self.trace = []
        self.opt = None
        self.anchor = []
        self.grads = {}       # parameter index -> the gradient it holds now
        self.keep = []        # every gradient ever given stays allocated, so no later buffer takes its address

    def roles(self):
        opt, out = self.opt, {}
        lists = [("param", opt.params), ("grad", self.grads), ("low", opt.low_words), ("anchor", self.anchor),
                 ("scale", opt._scales), ("acc", opt.accumulated_grads()), ("ema", opt.ema_tensors()),
                 ("exp_avg", opt.exp_avg), ("exp_avg_sq", opt.exp_avg_sq)]     # SGD's moment slots alias the parameters
        for role, ts in lists:
            for i, t in (ts.items() if isinstance(ts, dict) else enumerate(ts)):
                if t.data_ptr():
                    out.setdefault(t.data_ptr(), [role, i])
        out.setdefault(opt._norm_coef.data_ptr(), ["norm_coef", 0])
        if getattr(opt, "_ws", None) is not None:
            out.setdefault(opt._ws.data_ptr(), ["norm_ws", 0])
        return out

    def __call__(self, real):
        def recording(name, *args):
            roles = self.roles()

            def one(a):
                if isinstance(a, bool) or not isinstance(a, int):
                    return a
                if a in roles:
                    return roles[a]
                return "buffer" if a >= 1 << 32 else a           # a workspace or an output the call allocated
            entry = [name]
            k = SIDE_TABLES.get(name)
            rest = args
            if k is not None:
                n = args[1 + k]
                rows = _read_i64(args[0], 6 * n)
                entry.append([[one(v) for v in rows[6 * r:6 * r + 4]] + rows[6 * r + 4:6 * r + 6] for r in range(n)])
                entry.append([None if p is None else [one(v) for v in _read_i64(p, n)] for p in args[1:1 + k]])
                rest = args[1 + k:]
            entry += [one(a) for a in rest[:-1]] + ["stream"]
            self.trace.append(entry)
            return real(name, *args)
        return recording


def _run(case, monkeypatch):
    from lcv_hip import ops
    from lcv_hip.lib import LcvError
    kind, form, ema, det = case.split("-")
    master, m8, accum, with_anchor, f32 = FORMS[form]
    rec = _Recorder()
    for name in ("ops", "optim"):                 # whichever module binds `call` for the optimizers
        try:
            mod = __import__(f"lcv_hip.{name}", fromlist=[name])
        except ImportError:
            continue
        if hasattr(mod, "call"):
            monkeypatch.setattr(mod, "call", rec(mod.call))
    was_det, epoch0 = ops.is_deterministic(), ops.PARAM_EPOCH
    ops.set_deterministic(det == "det")
    try:
        dt = torch.float32 if f32 else torch.bfloat16
        params = [((torch.arange(n, dtype=torch.float32) % 7 - 3) / 8).to(dt).to(DEV) for n in NUMELS]
        rec.anchor = [p.clone() for p in params] if with_anchor else []
        kw = dict(weight_decay=0.01, master_weights=master, grad_accum=accum, anchor=rec.anchor or None)
        if kind == "sgd":
            opt = ops.FusedSGDClip(params, lr=1e-3, **kw)
        else:
            opt = ops.FusedAdamWClip(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, moments_8bit=m8, **kw)
        rec.opt = opt
        if ema == "ema":
            opt.enable_weight_ema(0.9, warmup=True)              # warm-up: the beta of every update differs
        for step in range(2):
            for micro in range(accum):
                for i in WITH_GRAD:
                    g = torch.full_like(params[i], 0.01 * (i + 1 + micro))
                    rec.keep.append(g)
                    rec.grads[i] = params[i].grad = g
                if accum > 1:
                    opt.accumulate()
            if step == 1:
                opt.clip_grad_norm_(1.0)
            opt.step()
            opt.zero_grad()
        if with_anchor:
            opt.drift_norm()
        if ema == "ema":
            opt.ema_swap()
            opt.ema_swap()
        for what in ("master_tensors", "moment_tensors"):        # refused without master weights / for SGD: recorded as such
            try:
                getattr(opt, what)()
            except LcvError:
                rec.trace.append([what, "refused"])
        torch.cuda.synchronize()
        rec.trace.append(["PARAM_EPOCH", ops.PARAM_EPOCH - epoch0])
    finally:
        ops.set_deterministic(was_det)
    return json.loads(json.dumps(rec.trace))


@pytest.mark.parametrize("case", list(_cases()))
def test_calls_and_tables_are_the_recorded_ones(case, monkeypatch):
    trace = _run(case, monkeypatch)
    if RECORD:
        golden = json.loads(GOLDEN.read_text()) if GOLDEN.exists() else {}
        golden[case] = trace
        body = ",\n".join(f"{json.dumps(k)}: {json.dumps(golden[k])}" for k in sorted(golden))
        GOLDEN.write_text("{\n" + body + "\n}\n")
    want = json.loads(GOLDEN.read_text())[case]
    assert [e[0] for e in trace] == [e[0] for e in want]
    for i, (got, exp) in enumerate(zip(trace, want)):
        assert got == exp, f"call {i} ({exp[0]})"


def test_the_golden_file_holds_exactly_these_cases():
    assert sorted(json.loads(GOLDEN.read_text())) == sorted(_cases())
