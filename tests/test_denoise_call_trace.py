"""CPU: what `LongCatVideoPipeline.denoise` hands to the model and to the step kernels, call by call.

The pipeline is built with a stub DiT (a deterministic function of its input, its timestep rows and its text row) and the real
scheduler on the host sigma grid, and runs 4 steps on CPU tensors with recording doubles over `ops.cfg_euler_step`,
`euler_step`, `cfg_lms_step`, `cfg_delta_store` and `cfg_delta_apply` that do the kernels' arithmetic in plain torch.  A trace
entry is the call's name, the step it belongs to, and per argument: a tensor as [shape, contiguous?, where its storage comes
from: "state" (the loop's latents), "pred" (this step's model output) or "own" (a copy or a buffer)], a scalar as it is.  Model
calls are recorded with their batch, input shape, timestep rows and whether the KV cache was handed in; the step callback is
recorded too, so the order update, store, callback is part of the trace.

The matrix: {conditioning frames pinned in the sequence, KV-cached, none} x {euler, ab2c} x {guided, guided with cfg_reuse=2,
unguided} (reuse needs guidance).  The golden file tests/golden/denoise_call_trace.json was written by this same file in record
mode (LCV_RECORD_DENOISE_TRACE=1) on the commit before the loop got its one update path; a rewrite of the loop must reproduce
it exactly."""
import json
import os
from pathlib import Path

import pytest
import torch

GOLDEN = Path(__file__).resolve().parent / "golden" / "denoise_call_trace.json"
RECORD = os.environ.get("LCV_RECORD_DENOISE_TRACE", "") == "1"
STEPS = 4
C, T, H, W = 4, 3, 4, 4
GUIDANCE = 4.0

LAYOUTS = {"pinned": (1, False), "kv": (1, True), "none": (0, True)}        # num_cond_latents, use_kv_cache
SOLVERS = ("euler", "ab2c")
MODES = ("guided", "guided+reuse2", "unguided")


def _cases():
    return [f"{lay}-{sol}-{mode}" for lay in LAYOUTS for sol in SOLVERS for mode in MODES]


class _Trace:
    def __init__(self):
        self.rows = []
        self.step = -1            # the step of the last model call
        self.pred = None          # storage of that call's output
        self.keep = []            # everything seen stays allocated: no later tensor takes a recorded address

    def tensor(self, t):
        if t is None:
            return None
        self.keep.append(t)
        return [list(t.shape), bool(t.is_contiguous()), t.untyped_storage().data_ptr()]

    def add(self, name, *args):
        self.rows.append([name, self.step] + [self.tensor(a) if (a is None or torch.is_tensor(a)) else a for a in args])

    def finish(self, state_storage):
        """Addresses -> "state" / "pred" / "own"; `pred` rows carry the address they are compared with and drop out."""
        out, pred = [], None

        def origin(a):
            if not (isinstance(a, list) and len(a) == 3 and isinstance(a[0], list)):
                return a
            return [a[0], a[1], "state" if a[2] == state_storage else "pred" if a[2] == pred else "own"]
        for row in self.rows:
            if row[0] == "(pred)":
                pred = row[2]
            else:
                out.append([origin(a) for a in row])
        return json.loads(json.dumps(out))


class _StubDiT:
    """pred = x / 4 + the text row's mean + the frame's timestep / 1000, fp32, shaped like the input."""

    def __init__(self, trace):
        self.trace = trace
        self.start = 0

    def __call__(self, hidden_states, timestep, encoder_hidden_states, encoder_attention_mask=None, num_cond_latents=0,
                 kv_cache_dict=None, return_kv=False, skip_crs_attn=False, **more):
        assert not more, sorted(more)
        tr = self.trace
        if return_kv:
            tr.add("dit_kv", list(hidden_states.shape), str(hidden_states.dtype), timestep.float().tolist(), skip_crs_attn)
            return None, {"stub": hidden_states.clone()}
        tr.step = self.start if tr.step < 0 else tr.step + 1
        B = hidden_states.shape[0]
        assert timestep.dtype == torch.bfloat16 and hidden_states.dtype == torch.bfloat16
        tr.add("dit", B, list(hidden_states.shape), bool(hidden_states.is_contiguous()), timestep.float().tolist(),
               list(encoder_hidden_states.shape), None if encoder_attention_mask is None else encoder_attention_mask.tolist(),
               int(num_cond_latents), kv_cache_dict is not None)
        text = encoder_hidden_states.float().mean(dim=(1, 2, 3)).view(B, 1, 1, 1, 1)
        pred = hidden_states.float() / 4 + text + timestep.float().view(B, 1, -1, 1, 1) / 1000
        pred = pred.contiguous()
        tr.keep.append(pred)
        tr.rows.append(["(pred)", tr.step, pred.untyped_storage().data_ptr()])
        return pred


def _guided(cond, uncond, guidance, zero_star):
    """The guided value in plain torch: u' = u * st, v = u' + g (c - u'), st = <c,u> / (<u,u> + 1e-8) per sample."""
    B = cond.shape[0]
    c, u = cond.reshape(B, -1), uncond.reshape(B, -1)
    if zero_star:
        st = (c * u).sum(1, keepdim=True) / ((u * u).sum(1, keepdim=True) + 1e-8)
        u = u * st
    return (u + guidance * (c - u)).reshape(cond.shape)


def _doubles(tr):
    def cfg_euler_step(cond, uncond, x, guidance, dt, negate=True, zero_star=True):
        tr.add("cfg_euler_step", cond, uncond, x, guidance, dt, negate, zero_star)
        v = _guided(cond, uncond, guidance, zero_star)
        x.add_((-v if negate else v).reshape(x.shape), alpha=dt)

    def euler_step(v, x, dt, negate=True):
        tr.add("euler_step", v, x, dt, negate)
        x.add_((-v if negate else v).reshape(x.shape), alpha=dt)

    def cfg_lms_step(cond, uncond, x, f0, f1, f2, guidance, weights, negate=True, zero_star=True):
        tr.add("cfg_lms_step", cond, uncond, x, f0, f1, f2, guidance, list(weights), negate, zero_star)
        v = cond if uncond is None else _guided(cond, uncond, guidance, zero_star)
        f0.copy_((-v if negate else v).reshape(f0.shape))
        for w, f in zip(weights, (f0, f1, f2)):
            x.add_(f, alpha=w)

    def cfg_delta_store(cond, uncond, delta, guidance, zero_star=True, out=None):
        tr.add("cfg_delta_store", cond, uncond, delta, guidance, zero_star, out)
        new = _guided(cond, uncond, guidance, zero_star) - cond
        if out is not None:
            B = delta.shape[0]
            out.view(B, 2)[:, 0] = (new - delta).abs().reshape(B, -1).sum(1)
            out.view(B, 2)[:, 1] = delta.abs().reshape(B, -1).sum(1)
        delta.copy_(new)

    def cfg_delta_apply(cond, delta, out=None):
        tr.add("cfg_delta_apply", cond, delta, out, None if out is None else out.data_ptr() == cond.data_ptr())
        if out is None:
            out = torch.empty_like(cond)
        torch.add(cond, delta, out=out)
        return out
    return dict(cfg_euler_step=cfg_euler_step, euler_step=euler_step, cfg_lms_step=cfg_lms_step, cfg_delta_store=cfg_delta_store,
                cfg_delta_apply=cfg_delta_apply)


def _run(case, monkeypatch):
    from lcv_hip import ops
    from longcat_video.modules.scheduling_flow_match_euler_discrete import FlowMatchEulerDiscreteScheduler
    from longcat_video.pipeline_longcat_video import LongCatVideoPipeline
    layout, solver, mode = case.split("-")
    ncl, use_kv = LAYOUTS[layout]
    monkeypatch.delenv("LCV_DENOISE_GRAPH", raising=False)
    monkeypatch.delenv("LCV_DENOISE_GRAPH_TOKENS", raising=False)
    tr = _Trace()
    for name, fn in _doubles(tr).items():
        monkeypatch.setattr(ops, name, fn)
    pipe = LongCatVideoPipeline(scheduler=FlowMatchEulerDiscreteScheduler(shift=3.0), dit=_StubDiT(tr))
    g = torch.Generator().manual_seed(7)
    lat = torch.randn((1, C, T, H, W), generator=g)
    pe = torch.randn((1, 1, 8, 16), generator=g).to(torch.bfloat16)
    ne = torch.randn((1, 1, 8, 16), generator=g).to(torch.bfloat16)
    pm, nm = torch.ones(1, 8, dtype=torch.int64), torch.tensor([[1] * 5 + [0] * 3])
    guided = mode != "unguided"
    state = []

    def callback(i, work):
        state.append(work.untyped_storage().data_ptr())
        tr.add("callback", i, work)
    kw = {}
    if solver != "euler":
        kw["solver"] = solver
    if mode == "guided+reuse2":
        kw["cfg_reuse"] = 2
    out = pipe.denoise(lat, pe, pm, ne if guided else None, nm if guided else None, num_cond_latents=ncl,
                       num_inference_steps=STEPS, guidance_scale=GUIDANCE if guided else 1.0, use_kv_cache=use_kv,
                       step_callback=callback, **kw)
    assert len(set(state)) == 1                      # one state tensor over the whole loop
    tr.rows.append(["return", STEPS, list(out.shape), pipe.scheduler._step_index,
                    None if pipe.last_cfg_reuse_stats is None else
                    {k: pipe.last_cfg_reuse_stats[k] for k in ("interval", "full", "reused", "reused_steps")}])
    if ncl:                                          # the conditioning frames come back untouched
        assert torch.equal(out[:, :, :ncl], lat[:, :, :ncl])
    return tr.finish(state[0])


@pytest.mark.parametrize("case", _cases())
def test_calls_are_the_recorded_ones(case, monkeypatch):
    trace = _run(case, monkeypatch)
    if RECORD:
        golden = json.loads(GOLDEN.read_text()) if GOLDEN.exists() else {}
        golden[case] = trace
        GOLDEN.write_text("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(golden[k])}" for k in sorted(golden)) + "\n}\n")
    want = json.loads(GOLDEN.read_text())[case]
    assert [e[:2] for e in trace] == [e[:2] for e in want]
    for i, (got, exp) in enumerate(zip(trace, want)):
        assert got == exp, f"call {i} ({exp[0]} of step {exp[1]})"


def test_the_golden_file_holds_exactly_these_cases():
    assert sorted(json.loads(GOLDEN.read_text())) == sorted(_cases())
