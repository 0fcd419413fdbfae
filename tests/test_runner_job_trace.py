"""CPU: the per-video job loop of the seven TTA runner scripts, call by call and file by file.

Every script's `main` runs over four synthetic entries with recording stand-ins for everything heavy: the distributed set-up,
the model and pipeline, the entry listing and loading, the augmentation variants, the continuation, scoring, saving, the early
stopper's `setup`, the checkpointing choice, `torch.cuda.synchronize`, and the method's own loop / adapter / wrapper calls.
`dp.write_checkpoint` is recorded and still writes.  A case's trace holds the ordered stand-in calls (name plus a brief form of
their arguments), the job's stdout (with the `12.3s` tokens of the per-video line masked) and `config.json`, `summary.json` and
`checkpoint.json`, where every value under a key ending in `_time` - and no other - is replaced by its type's name.  The times
themselves are asserted on the unmasked rows: the continuation stand-in reports 7.0 s, the LoRA / full loops report 3.0 s.

Cases per script: `job` (entry 1 fails to load, entry 2 fails in the continuation: two error rows, the job goes on), `resume`
(the same output directory again: nothing left to do), `restart` (the runners with the flag: everything again), `fatal` (entry
3 raises an exception whose `fatal` is true: checkpoint at 3, re-raised), and three runs over one video with the flags that
add keys.

The golden file tests/golden/runner_job_trace.json was written by this same file in record mode (LCV_RECORD_RUNNER_TRACE=1) on
the commit before the three loops became one driver.  The comparison ignores key order inside JSON objects and is otherwise
exact: key sets, value types and values at every level, and the order of the calls."""
import importlib.util
import json
import os
import re
import sys
import types
from pathlib import Path

import pytest
import torch
from torch import nn

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "longcat-video-tta_amd"
if str(PKG) not in sys.path:
    sys.path.insert(0, str(PKG))
GOLDEN = Path(__file__).resolve().parent / "golden" / "runner_job_trace.json"
RECORD = os.environ.get("LCV_RECORD_RUNNER_TRACE", "") == "1"

LORA, FULL = "lora_experiment/scripts/run_lora_tta.py", "lora_experiment/scripts/run_full_tta.py"
NORM = "delta_experiment/scripts/run_norm_tune_tta.py"
DELTA = ["delta_experiment/scripts/run_delta_a.py", "delta_experiment/scripts/run_delta_b.py",
         "delta_experiment/scripts/run_delta_c.py", "delta_experiment/scripts/run_film_tta.py", NORM]
SCRIPTS = [LORA, FULL] + DELTA
# 33 pixel frames -> 9 latent frames: 4 context, 4 train, 1 held out (the early stopper is on)
BASE = ["--checkpoint-dir", "stub", "--data-dir", "stub", "--num-cond-frames", "13", "--tta-total-frames", "33",
        "--gen-start-frame", "33", "--device", "cpu"]
METHOD_FLAGS = {LORA: ["--save-lora-weights", "--use-builtin-lora"],
                FULL: ["--master-weights", "--decay-to-base", "--weight-ema", "0.9"],
                NORM: ["--master-weights", "--decay-to-base", "--weight-ema", "0.9"]}


class _Fatal(RuntimeError):
    fatal = True


class _Attn(nn.Module):
    def __init__(self):
        super().__init__()
        self.q_norm, self.k_norm = nn.LayerNorm(2), nn.LayerNorm(2)


class _Block(nn.Module):
    def __init__(self):
        super().__init__()
        self.adaLN_modulation, self.pre_crs_attn_norm = nn.Linear(2, 2), nn.LayerNorm(2)
        self.attn, self.cross_attn = _Attn(), _Attn()


class _TinyDiT(nn.Module):
    """The attributes the wrappers' constructors touch."""

    def __init__(self):
        super().__init__()
        self.config = types.SimpleNamespace(adaln_tembed_dim=4, hidden_size=4, out_channels=16, in_channels=16, caption_channels=4)
        self.t_embedder, self.final_layer = nn.Linear(2, 2), nn.Linear(2, 2)
        self.blocks = nn.ModuleList([_Block(), _Block()])


def _brief(v):
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, _TinyDiT):
        return "dit"
    if isinstance(v, nn.Module):
        return type(v).__name__
    if torch.is_tensor(v):
        return f"{str(v.dtype).replace('torch.', '')}{list(v.shape)}"
    if isinstance(v, (list, tuple)):
        return [(x["name"] if isinstance(x, dict) and "name" in x else _brief(x)) for x in v]
    if isinstance(v, dict):
        return {"dict": sorted(map(str, v))}
    if callable(v):
        return "callable"
    return type(v).__name__


class _Job:
    """The stand-ins of one `main` call and what they saw."""

    def __init__(self, fail_load=(), fail_gen=(), fatal_gen=()):
        self.calls = []
        self.fail_load, self.fail_gen, self.fatal_gen = set(fail_load), set(fail_gen), set(fatal_gen)

    def add(self, name, *args, **kw):
        self.calls.append([name] + [_brief(a) for a in args] + ([{k: _brief(kw[k]) for k in sorted(kw)}] if kw else []))

    # ---- the shared pieces
    def setup_distributed(self, args):       # not recorded: a runner that sets itself up inline never comes through here
        return 0, 1, "cpu"

    def load_components(self, args, device):
        self.add("load_components", device)
        job = self

        class _Pipe:
            vae = object()

            def decode_to_frames(self, out):
                job.add("decode_to_frames", out)
                return torch.zeros(4, 8, 8, 3)
        return _TinyDiT(), _Pipe()

    def list_eval_entries(self, args, dit):
        self.add("list_eval_entries", dit)
        return [{"kind": "stub", "name": f"clip_{i}", "path": f"stub://clip_{i}", "seed": i} for i in range(min(4, args.max_videos))]

    def load_entry(self, entry, args, dit, device, total_frames=None, pipe=None):
        self.add("load_entry", entry["name"], dit, device, pipe=type(pipe).__name__)
        if entry["seed"] in self.fail_load:
            raise RuntimeError(f"stand-in: {entry['name']} cannot be loaded")
        return {"latents": torch.zeros(1, 16, 9, 4, 4, dtype=torch.bfloat16), "prompt_embeds": torch.zeros(1, 1, 4, 4),
                "prompt_mask": torch.ones(1, 4, dtype=torch.int64), "caption": f"caption of {entry['name']}"}

    def train_latents_variants_for(self, args, pipe, blob, entry, cond, train, device):
        self.add("train_latents_variants_for", entry["name"], cond, train, device)
        return cond, train, ([{"name": "orig"}, {"name": "hflip"}] if args.aug_enabled else None)

    def generate_continuation(self, pipe, blob, args, idx, device, num_frames=None, entry=None):
        self.add("generate_continuation", idx, device, entry=entry["name"])
        if idx in self.fatal_gen:
            raise _Fatal(f"stand-in: device error in the continuation of video {idx}")
        if idx in self.fail_gen:
            raise RuntimeError(f"stand-in: the continuation of video {idx} failed")
        blob["_cond_source"] = "stand_in_cond"
        if args.step_cache is not None:
            blob["_step_cache"] = {"computed": 3, "skipped": 1}
        if args.cfg_reuse is not None:
            blob["_cfg_reuse"] = {"full": 2, "reused": 2}
        return torch.zeros(1, 16, 4, 4, 4), 7.0

    def score_generation(self, frames, blob, entry, args, num_frames=None, flavour="tta"):
        self.add("score_generation", frames, entry["name"], flavour)
        return {"psnr": 30.0 + entry["seed"], "ssim": 0.5 + entry["seed"] / 8, "lpips": None}

    def save_frames(self, pipe, latents, path_noext, frames=None, fps=24):
        self.add("save_frames", os.path.basename(path_noext), Path(path_noext).parent.name, frames)
        return os.path.basename(path_noext) + ".npy"        # a row's output_path: kept free of the temporary directory

    def choose_gradient_checkpointing(self, dit, n_tokens, *a, **kw):
        self.add("choose_gradient_checkpointing", dit, n_tokens, *a, **kw)

    def es_setup(self, stopper, *a, **kw):
        named = dict(zip(("model", "cond_latents", "val_latents", "prompt_embeds", "prompt_mask"), a))
        assert not set(named) & set(kw)
        self.add("es.setup", **named, **kw)

    def synchronize(self, *a, **kw):
        self.add("cuda.synchronize")

    # ---- the methods' own
    def _loop(self, name, model, args, kw, extra):
        self.add(name, model, *args, **kw)
        return {"losses": [0.5, 0.25], "es_check_time": 0.125,
                "early_stopping_info": {"stopped_early": False, "best_step": 2, "best_val_loss": 0.25}, **extra}

    def finetune_lora_on_conditioning(self, dit, lora_modules, *args, **kw):
        return self._loop("finetune_lora_on_conditioning", dit, (len(lora_modules),) + args, kw, {"train_time": 3.0})

    def finetune_full_on_conditioning(self, dit, *args, **kw):
        return self._loop("finetune_full_on_conditioning", dit, args, kw,
                          {"train_time": 3.0, **({"drift_norm": 0.5} if kw.get("decay_to_base") else {})})

    def optimizer_of(self, name, **extra):
        return lambda w, *args, **kw: self._loop(name, w, args, kw, extra)

    def optimize_norm_params(self, w, params, *args, **kw):
        return self._loop("optimize_norm_params", w, (len(params),) + args, kw,
                          {"norm_param_drift": 0.0625, **({"delta_norm": 0.25} if w.delta is not None else {}),
                           **({"drift_norm": 0.5} if kw.get("decay_to_base") else {})})

    def recorder(self, name, result=None, brief=lambda a, kw: (a, kw)):
        def call(*a, **kw):
            a2, kw2 = brief(a, kw)
            self.add(name, *a2, **kw2)
            return result() if callable(result) else result
        return call


def _load_script(rel):
    path = PKG / rel
    spec = importlib.util.spec_from_file_location("job_trace_" + path.stem, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _install(mp, mod, job):
    """Attach the stand-ins by name wherever the name lives: the script module, tta.runner_common and the defining module."""
    from longcat_video.parallel import data_parallel as dp
    from tta import delta, early_stopping, inner_loop
    from tta import runner_common as R

    def put(name, fn, *homes):
        hit = False
        for m in (mod, R) + homes:
            if hasattr(m, name):
                mp.setattr(m, name, fn)
                hit = True
        assert hit, name

    for name in ("setup_distributed", "load_components", "list_eval_entries", "load_entry", "train_latents_variants_for",
                 "generate_continuation", "score_generation", "save_frames"):
        put(name, getattr(job, name))
    put("choose_gradient_checkpointing", job.choose_gradient_checkpointing, inner_loop)
    mp.setattr(early_stopping.AnchoredEarlyStopper, "setup", lambda self, *a, **kw: job.es_setup(self, *a, **kw))
    mp.setattr(torch.cuda, "synchronize", job.synchronize)
    real_write = dp.write_checkpoint

    def write_checkpoint(output_dir, next_idx, results, rank=None):
        job.add("write_checkpoint", next_idx, len(results), rank=rank)
        return real_write(output_dir, next_idx, results, rank=rank)
    mp.setattr(dp, "write_checkpoint", write_checkpoint)

    rel = next(r for r in SCRIPTS if mod.__file__.endswith(r))
    first = lambda a, kw: (a[:1], kw)                         # the model, not the list of adapter modules
    count = lambda a, kw: ((len(a[0]),) + a[1:], kw)
    named = lambda a, kw: ((len(a[0]), os.path.basename(a[1]), Path(a[1]).parent.name), kw)
    if rel == LORA:
        put("finetune_lora_on_conditioning", job.finetune_lora_on_conditioning)
        for pre in ("", "builtin_"):
            put(f"inject_{pre}lora_into_dit", job.recorder(f"inject_{pre}lora_into_dit", lambda: [nn.Linear(2, 2), nn.Linear(2, 2)], first))
            put(f"count_{pre}lora_parameters", job.recorder(f"count_{pre}lora_parameters", {"total_lora": 24, "trainable": 12}, count))
            put(f"reset_{pre}lora_weights", job.recorder(f"reset_{pre}lora_weights", None, count))
            put(f"save_{pre}lora_weights", job.recorder(f"save_{pre}lora_weights", None, named))
    elif rel == FULL:
        put("finetune_full_on_conditioning", job.finetune_full_on_conditioning)
        put("snapshot_base_state", job.recorder("snapshot_base_state", lambda: {"w": torch.zeros(1)}))
        put("reset_dit_weights", job.recorder("reset_dit_weights"))
    else:
        extras = {"optimize_delta_a": {"delta_norm": 0.25}, "optimize_delta_b": {"delta_norms": [0.25, 0.5, 0.0, 0.0]},
                  "optimize_delta_c": {"delta_out_norm": 0.125}, "optimize_film_adapter": {"correction_norm": 0.75}}
        for name, extra in extras.items():
            if hasattr(mod, name):
                put(name, job.optimizer_of(name, **extra))
        if rel == NORM:
            put("optimize_norm_params", job.optimize_norm_params)
        for cls in (delta._HookedWrapper, delta.NormTuneForward):
            mp.setattr(cls, "remove_from_dit", lambda self: job.add("remove_from_dit", self))
        for cls in (delta.DeltaAWrapper, delta.DeltaBWrapper, delta.DeltaCWrapper, delta.FiLMAdapterWrapper, delta.NormTuneForward):
            mp.setattr(cls, "apply_to_dit", lambda self: job.add("apply_to_dit", self))
        mp.setattr(delta.NormTuneForward, "restore", lambda self: job.add("restore", self))


def _mask(v):
    if isinstance(v, dict):
        return {k: (type(x).__name__ if k.endswith("_time") else _mask(x)) for k, x in v.items()}
    return [_mask(x) for x in v] if isinstance(v, list) else v


def _check_times(rel, rows, skipped_generation):
    """The times of the successful rows, compared as numbers: the stand-in continuation's 7.0 s is real, decode and scoring
    take next to nothing; the LoRA / full loops report their own 3.0 s, the delta family's is wall time around a stand-in."""
    for r in rows:
        if not r["success"]:
            assert not any(k.endswith("_time") for k in r), r
            continue
        gen = r.get("gen_time", 0.0)
        assert r["total_time"] == r["train_time"] + gen, r
        assert ("gen_time" in r) is (not skipped_generation), r
        if not skipped_generation:
            assert 7.0 <= gen < 7.5, r
        if rel in (LORA, FULL):
            assert r["train_time"] == 3.0, r
        else:
            assert 0 <= r["train_time"] < 0.5, r
        assert r["es_check_time"] == 0.125, r


def _run(rel, mod, out, flags, capsys, **fails):
    """One `main` call under the stand-ins: calls, stdout, the three files (masked), and the exception if one came out."""
    job = _Job(**fails)
    capsys.readouterr()
    raised = None
    with pytest.MonkeyPatch.context() as mp:
        _install(mp, mod, job)
        try:
            mod.main(BASE + ["--output-dir", str(out)] + flags)
        except _Fatal as ex:
            raised = f"{type(ex).__name__}: {ex}"
    stdout = [re.sub(r"\b\d+\.\ds\b", "#s", ln).replace(str(out), "<out>") for ln in capsys.readouterr().out.splitlines()]
    files = {}
    for name in ("config.json", "summary.json", "checkpoint.json"):
        files[name] = json.loads((out / name).read_text()) if (out / name).exists() else None
    _check_times(rel, files["checkpoint.json"]["results"], "--skip-generation" in flags)
    if files["summary.json"] is not None:
        _check_times(rel, files["summary.json"]["results"], "--skip-generation" in flags)
    others = sorted(str(p.relative_to(out)) for p in out.rglob("*") if p.name not in files)
    return json.loads(json.dumps({"calls": job.calls, "stdout": stdout, "raised": raised, "other_paths": others,
                                  "files": _mask(files)}))


def _trace(rel, tmp_path, capsys):
    mod = _load_script(rel)
    fails = dict(fail_load=[1], fail_gen=[2])
    method = METHOD_FLAGS.get(rel, [])
    t = {"job": _run(rel, mod, tmp_path / "a", [], capsys, **fails),
         "resume": _run(rel, mod, tmp_path / "a", [], capsys, **fails)}
    if rel in (LORA, FULL):
        t["restart"] = _run(rel, mod, tmp_path / "a", ["--restart"], capsys, **fails)
    t["fatal"] = _run(rel, mod, tmp_path / "b", [], capsys, fatal_gen=[3], **fails)
    one = ["--max-videos", "1"]             # the flags that add keys: one video shows them
    t["flags_cache"] = _run(rel, mod, tmp_path / "c", one + ["--step-cache", "0.1", "--step-cache-max-skip", "2", "--solver", "ab2c",
                                                             "--aug-enabled"] + method, capsys)
    t["flags_reuse"] = _run(rel, mod, tmp_path / "d", one + ["--cfg-reuse", "2", "--cfg-reuse-warmup", "1", "--no-save-videos"]
                            + (["--also-tune-delta"] if rel == NORM else []), capsys)
    t["flags_skip"] = _run(rel, mod, tmp_path / "e", one + ["--skip-generation", "--es-disable"], capsys)
    return t


def _fold(t):
    """What is written twice is said once, so that the golden file stays readable: checkpoint.json's rows where they are
    summary.json's, a later case's calls, stdout or files where they are the `job` case's, and the head that the `fatal`
    case's calls and rows share with the `job` case's."""
    def after_shared_head(seq, ref, what):
        n = next((i for i, (a, b) in enumerate(zip(seq, ref)) if a != b), min(len(seq), len(ref)))
        return [f"= the first {n} {what} of job"] + seq[n:]
    job_rows = t["job"]["files"]["summary.json"]["results"]
    for case in t.values():
        summary, checkpoint = case["files"]["summary.json"], case["files"]["checkpoint.json"]
        if summary is not None and checkpoint["results"] == summary["results"]:
            checkpoint["results"] = "= the results of summary.json"
    fatal = t["fatal"]
    fatal["files"]["checkpoint.json"]["results"] = after_shared_head(fatal["files"]["checkpoint.json"]["results"], job_rows, "rows")
    fatal["calls"] = after_shared_head(fatal["calls"], t["job"]["calls"], "calls")
    for name, case in t.items():
        for part in ("calls", "stdout", "files"):
            if name != "job" and case[part] == t["job"][part]:
                case[part] = "= job"
    return t


def _same(got, want, where):
    """Equal up to the order of a JSON object's keys; 1, 1.0 and True are three different values."""
    assert type(got) is type(want), f"{where}: {got!r} is not the {type(want).__name__} {want!r}"
    if isinstance(want, dict):
        assert sorted(got) == sorted(want), f"{where}: keys {sorted(got)} != {sorted(want)}"
        for k in want:
            _same(got[k], want[k], f"{where}.{k}")
    elif isinstance(want, list):
        assert len(got) == len(want), f"{where}: {len(got)} entries, not {len(want)}:\n{got}\n{want}"
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, f"{where}[{i}]")
    else:
        assert got == want, f"{where}: {got!r} != {want!r}"


@pytest.mark.parametrize("rel", SCRIPTS)
def test_the_job_loop_reproduces_the_recorded_trace(rel, tmp_path, capsys):
    got = _trace(rel, tmp_path, capsys)
    # what the cases are there to show, said once outright
    nexts = lambda case: [c[1] for c in got[case]["calls"] if c[0] == "write_checkpoint"]
    assert nexts("job") == [1, 2, 3, 4, 4] and nexts("resume") == [4] and nexts("fatal") == [1, 2, 3, 3]
    assert [r["success"] for r in got["job"]["files"]["summary.json"]["results"]] == [True, False, False, True]
    assert got["fatal"]["raised"] and got["fatal"]["files"]["summary.json"] is None
    assert got["fatal"]["files"]["checkpoint.json"]["next_idx"] == 3
    if "restart" in got:
        assert nexts("restart") == nexts("job")
    got = _fold(got)
    if RECORD:
        golden = json.loads(GOLDEN.read_text()) if GOLDEN.exists() else {}
        golden[rel] = got
        GOLDEN.write_text(_dump(golden))
        return
    _same(got, json.loads(GOLDEN.read_text())[rel], rel)


def _dump(golden):
    """One line per part of a case."""
    line = lambda v: json.dumps(v, sort_keys=True, separators=(",", ":"))
    scripts = []
    for rel in sorted(golden):
        cases = []
        for name in sorted(golden[rel]):
            parts = ",\n".join(f'   {json.dumps(k)}: {line(v)}' for k, v in sorted(golden[rel][name].items()))
            cases.append(f'  {json.dumps(name)}: {{\n{parts}\n  }}')
        scripts.append(f' {json.dumps(rel)}: {{\n' + ",\n".join(cases) + "\n }")
    return "{\n" + ",\n".join(scripts) + "\n}\n"
