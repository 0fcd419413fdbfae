"""LPIPS v0.1 with the AlexNet backbone, on the device — the third quality column of every result row.

The reference builds `lpips.LPIPS(net="alex")` once and calls it on each generated / ground-truth frame pair
(delta_experiment/scripts/common.py:648-660, 740-757; baseline_experiment/scripts/run_baseline.py:148-165, 442).  Here
the network is five MFMA convolutions, two pools and five tap distances of liblcv_hip.so (`lcv_hip.ops.lpips_alex`,
include/lcv_hip_lpips.h); this module owns the weights: reading them from the files the two packages ship, checking
every tensor, and packing them once into the layout the kernels read.  What is assumed about the two packages is
itemised in spec/lpips.md.

Opt-in: the runners resolve a model from the environment variable `LCV_LPIPS_WEIGHTS` (`model_from_env`) — a path, or
`synthetic:<seed>` for plumbing runs.  Unset, the column stays null, which is the reference's own behaviour when the
package is not importable.
"""
import os
from pathlib import Path
from typing import Dict, Optional

import torch

from lcv_hip import ops

ENV_VAR = "LCV_LPIPS_WEIGHTS"
# torchvision's `features` index of each convolution, and the slice each lands in inside lpips' wrapper (spec/lpips.md L6)
_TV_INDEX = (0, 3, 6, 8, 10)
_LPIPS_CONV_KEYS = tuple(f"net.slice{i + 1}.{j}" for i, j in enumerate(_TV_INDEX))
_TV_CONV_KEYS = tuple(f"features.{j}" for j in _TV_INDEX)
_LIN_KEYS = tuple(f"lin{i}.model.1.weight" for i in range(5))


def _conv_shapes():
    return [((cout, cin, k, k), (cout,)) for cin, cout, k, _, _, _ in ops.LPIPS_ALEX_LAYERS]


def _take(sd: Dict[str, torch.Tensor], key: str, shape, source: str) -> torch.Tensor:
    if key not in sd:
        raise KeyError(f"LPIPS weights: key {key!r} is missing from {source}")
    t = torch.as_tensor(sd[key])
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"LPIPS weights: {key!r} in {source} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t.detach().to(torch.float32)


def _load_file(path: Path) -> Dict[str, torch.Tensor]:
    sd = torch.load(str(path), map_location="cpu", weights_only=True)
    if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
        sd = sd["state_dict"]
    if not isinstance(sd, dict):
        raise ValueError(f"LPIPS weights: {path} does not hold a state dict")
    return sd


def merge_backbone_and_lin(backbone: Dict[str, torch.Tensor], lin: Dict[str, torch.Tensor],
                           source: str = "torchvision AlexNet + lin file") -> Dict[str, torch.Tensor]:
    """torchvision's `features.{0,3,6,8,10}.*` + the package's `lin{0..4}.model.1.weight` -> the one-file layout."""
    out = {}
    for tv, lp in zip(_TV_CONV_KEYS, _LPIPS_CONV_KEYS):
        for leaf in ("weight", "bias"):
            if f"{tv}.{leaf}" not in backbone:
                raise KeyError(f"LPIPS weights: key {tv + '.' + leaf!r} is missing from {source}")
            out[f"{lp}.{leaf}"] = backbone[f"{tv}.{leaf}"]
    for k in _LIN_KEYS:
        if k not in lin:
            raise KeyError(f"LPIPS weights: key {k!r} is missing from {source}")
        out[k] = lin[k]
    return out


def check_state_dict(state: Dict[str, torch.Tensor], source: str = "state dict") -> Dict[str, torch.Tensor]:
    """Every tensor the network needs, present and of the right shape, as fp32 (host side: no GPU involved)."""
    out = {}
    for (wshape, bshape), ckey, lkey in zip(_conv_shapes(), _LPIPS_CONV_KEYS, _LIN_KEYS):
        out[ckey + ".weight"] = _take(state, ckey + ".weight", wshape, source)
        out[ckey + ".bias"] = _take(state, ckey + ".bias", bshape, source)
        out[lkey] = _take(state, lkey, (1, wshape[0], 1, 1), source)
    if "scaling_layer.shift" in state or "scaling_layer.scale" in state:
        out["scaling_layer.shift"] = _take(state, "scaling_layer.shift", (1, 3, 1, 1), source)
        out["scaling_layer.scale"] = _take(state, "scaling_layer.scale", (1, 3, 1, 1), source)
    return out


def read_state_dict(path, lin_path=None):
    """(a) one file in the `lpips.LPIPS(net="alex").state_dict()` layout; (b) a directory holding torchvision's AlexNet
    file (`alexnet*.pth`) and the package's `alex.pth`, or the two files given as `path`, `lin_path`.  Returns the
    checked one-file layout and a description of where it came from; a missing key or a wrong shape raises, named."""
    path = Path(path)
    if lin_path is None and path.is_dir():
        nets = sorted(path.glob("alexnet*.pth"))
        if not (path / "alex.pth").exists() or not nets:
            raise FileNotFoundError(f"LPIPS weights: {path} must hold alexnet*.pth (torchvision) and alex.pth (lpips lin layers)")
        path, lin_path = nets[0], path / "alex.pth"
    if lin_path is not None:
        source = f"{path} + {lin_path}"
        return check_state_dict(merge_backbone_and_lin(_load_file(path), _load_file(Path(lin_path)), source), source), source
    return check_state_dict(_load_file(path), str(path)), str(path)


class LpipsAlex:
    """The packed device weights of LPIPS-alex; calling it scores frame pairs."""

    def __init__(self, state: Dict[str, torch.Tensor], device="cuda", source: str = "state dict"):
        """`state`: the `lpips.LPIPS(net="alex").state_dict()` layout (CPU or GPU tensors)."""
        state = check_state_dict(state, source)
        conv, lin = [], []
        for ckey, lkey in zip(_LPIPS_CONV_KEYS, _LIN_KEYS):
            conv.append((ops.lpips_pack_weight(state[ckey + ".weight"].to(device)), state[ckey + ".bias"].to(device).contiguous()))
            lin.append(state[lkey].to(device).reshape(-1).contiguous())
        shift, scale = ops.LPIPS_SHIFT, ops.LPIPS_SCALE
        if "scaling_layer.shift" in state:
            shift = tuple(float(v) for v in state["scaling_layer.shift"].reshape(-1))
            scale = tuple(float(v) for v in state["scaling_layer.scale"].reshape(-1))
        self.weights = ops.LpipsWeights(conv, lin, shift, scale)
        self.source = source

    # ---- construction --------------------------------------------------
    @classmethod
    def load(cls, path, lin_path=None, device="cuda") -> "LpipsAlex":
        """Weights from disk (`read_state_dict` describes the accepted layouts), packed onto `device`."""
        state, source = read_state_dict(path, lin_path)
        return cls(state, device, source=source)

    @staticmethod
    def synthetic_state_dict(seed: int) -> Dict[str, torch.Tensor]:
        """Random-init weights of the real architecture, drawn on a CPU generator in a fixed order so that a test can
        rebuild them: per layer He-normal convolution weights (std sqrt(2 / fan_in)), biases N(0, 0.05²), then
        non-negative lin weights U[0,1) * 2 / C (the shipped lin layers are non-negative)."""
        g = torch.Generator().manual_seed(int(seed))
        sd = {}
        for i, ((wshape, bshape), ckey, lkey) in enumerate(zip(_conv_shapes(), _LPIPS_CONV_KEYS, _LIN_KEYS)):
            fan_in = wshape[1] * wshape[2] * wshape[3]
            sd[ckey + ".weight"] = torch.randn(wshape, generator=g) * (2.0 / fan_in) ** 0.5
            sd[ckey + ".bias"] = torch.randn(bshape, generator=g) * 0.05
            sd[lkey] = torch.rand((1, wshape[0], 1, 1), generator=g) * (2.0 / wshape[0])
        return sd

    @classmethod
    def synthetic(cls, seed: int = 0, device="cuda") -> "LpipsAlex":
        return cls(cls.synthetic_state_dict(seed), device, source=f"synthetic:{int(seed)}")

    # ---- evaluation ----------------------------------------------------
    def __call__(self, gen: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
        """gen fp32 [N,H,W,3] in [0,1], gt fp32 or uint8 of the same shape -> fp32 [N] per-frame LPIPS (device)."""
        return ops.lpips_alex(gen, gt, self.weights)


_ENV_MODEL = {}


def model_from_env(device="cuda") -> Optional[LpipsAlex]:
    """The process-wide model named by LCV_LPIPS_WEIGHTS (a weights path, or `synthetic:<seed>`), built once per value;
    None when the variable is unset or empty — the result rows then keep `lpips: null`."""
    spec = os.environ.get(ENV_VAR, "").strip()
    if not spec:
        return None
    key = (spec, str(device))
    if key not in _ENV_MODEL:
        if spec.startswith("synthetic:"):
            _ENV_MODEL[key] = LpipsAlex.synthetic(int(spec.split(":", 1)[1]), device)
        else:
            _ENV_MODEL[key] = LpipsAlex.load(spec, device=device)
    return _ENV_MODEL[key]
