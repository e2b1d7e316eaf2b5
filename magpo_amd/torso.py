"""The actor's torso configuration: ``network.actor_network.pre_torso`` / ``post_torso`` (rec_magpo.py:570-579) as the
``MLPTorso(layer_sizes, activation, use_layer_norm, activate_final)`` they instantiate (mava/networks/torsos.py:24-47).

Per layer: ``x = Dense(width)(x)``, then ``LayerNorm(use_scale=False)`` when ``use_layer_norm``, then the activation on every layer
but the last, and on the last when ``activate_final``.  What the gfx950 kernels cover is checked here; anything else raises.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Tuple

MLP_TARGET = "mava.networks.torsos.MLPTorso"
WIDTHS = (64, 128, 192, 256)     # row widths of the dense / LayerNorm kernels (magpo_linear KIN, magpo_ln_act_*)
MAX_LAYERS = 3
ACT_CODES = {"relu": 1, "tanh": 5}   # magpo_linear / magpo_ln_act_* activation codes (include/magpo.h)


@dataclass(frozen=True)
class TorsoSpec:
    layer_sizes: Tuple[int, ...] = (128,)
    activation: str = "relu"
    use_layer_norm: bool = False
    activate_final: bool = True

    def __post_init__(self):
        sizes = tuple(int(w) for w in self.layer_sizes)
        object.__setattr__(self, "layer_sizes", sizes)
        if not 1 <= len(sizes) <= MAX_LAYERS:
            raise NotImplementedError(f"actor torso: 1 to {MAX_LAYERS} layers supported, got layer_sizes={list(sizes)}")
        bad = [w for w in sizes if w not in WIDTHS]
        if bad:
            raise NotImplementedError(f"actor torso: layer widths must be in {WIDTHS} (the gfx950 row / dense kernels), got {bad}")
        if self.activation not in ACT_CODES:
            raise NotImplementedError(f"actor torso: activation must be relu or tanh, got {self.activation!r}")
        object.__setattr__(self, "use_layer_norm", bool(self.use_layer_norm))
        object.__setattr__(self, "activate_final", bool(self.activate_final))

    @property
    def width(self) -> int:
        """Width of the torso's output."""
        return self.layer_sizes[-1]

    def act(self, i: int) -> int:
        """Activation code of layer i (0: none)."""
        return ACT_CODES[self.activation] if (i < len(self.layer_sizes) - 1 or self.activate_final) else 0


DEFAULT_TORSO = TorsoSpec()


def torso_from_config(cfg: Any) -> TorsoSpec:
    """A TorsoSpec from one ``actor_network.pre_torso`` / ``post_torso`` node (Config or dict)."""
    d = cfg.to_container() if hasattr(cfg, "to_container") else dict(cfg)
    target = d.get("_target_", MLP_TARGET)
    if target != MLP_TARGET:
        raise NotImplementedError(f"actor torso: only {MLP_TARGET} is supported on the HIP path, got _target_={target!r}")
    unknown = set(d) - {"_target_", "layer_sizes", "activation", "use_layer_norm", "activate_final"}
    if unknown:
        raise NotImplementedError(f"actor torso: unsupported MLPTorso keys {sorted(unknown)}")
    sizes = d.get("layer_sizes")
    if isinstance(sizes, (int, str)) or sizes is None:
        raise NotImplementedError(f"actor torso: layer_sizes must be a list of widths, got {sizes!r}")
    return TorsoSpec(tuple(sizes), str(d.get("activation", "relu")), bool(d.get("use_layer_norm", False)),
                     bool(d.get("activate_final", True)))


def layer_name(prefix: str, i: int) -> str:
    """Parameter-name stem of layer i of the ``pre`` / ``post`` torso: ``pre``, ``pre1``, ``pre2`` (layer 0 keeps the historical name)."""
    return prefix if i == 0 else f"{prefix}{i}"
