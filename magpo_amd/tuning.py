"""Per-call tuning knobs of the C ABI, held on the HOST side.

libmagpo_hip.so has no setters, reads no environment variables and keeps no state that changes results or buffer
sizes (include/magpo.h, conventions): every knob below is an argument of the entry points it affects.  The host
objects (SableGuider, GruActor) own one ``Tuning`` and pass its fields on every call, so two learners in one process
can run under different settings and a forward / backward pair can never see different values.

Environment variables are read HERE, once, when the default instance is built (A/B measurements from the shell):
    MAGPO_RET_CHUNK=64          retention chunk kernels on 64-token chunks (default 32)
    MAGPO_GRU_SPLIT_BF16=0|1|2  GRU training scans: 2 (default) = the forward scan's recurrent GEMM on bf16 MFMA with operands split in THREE pieces (24
                                mantissa bits = fp32 operands, six products, fp32 accumulate: error against fp64 no larger than the fp32-MFMA scan's,
                                tests/test_kernels_gpu.py::test_gru_scan_bf16_triples_keep_fp32_accuracy), backward on fp32 MFMA; 0 = fp32 MFMA everywhere;
                                1 = pairs (16 mantissa bits, forward and backward; never a default)
    MAGPO_GRU_BLOCK_ROWS=32|64  recurrent rows per workgroup of the fp32 GRU scans (default: by size)
    MAGPO_LINEAR_BF3=1          dense layers with 128 / 192 inputs (four-wave column blocks) on bf16 MFMA with three-piece operand splits (24 mantissa bits,
                                error against fp64 no larger than the fp32-MFMA kernel's, test_linear_bf16_triples_keep_fp32_accuracy).  OPT-IN: on the
                                3x30-50 sweep the runs with it on the actor ended at 90.5 (ten seeds) against 93.4 without
                                (profiles/r03_sweep_return_at_10M.md) -- not understood, so not a default
    MAGPO_WGRAD_BF3=1           the 128 x 384 weight gradient on bf16 triples: opt-in, its accumulation error is 1.2 x the fp32-MFMA kernel's
    MAGPO_ACT_EPW=4|8|16        envs per wave of the fused acting kernel (default: by size)
    MAGPO_PPO_FUSED_STEP=0|1    acting step of rec_ippo / rec_mappo: 1 = both GRU cells in one magpo_gru_cell_step launch (csrc/gru_step.hip), 0 = the
                                composed GruActor.step of each network (magpo_linear for xi + a T = 1 scan).  Same function, fp32 summation order differs.
                                Default: see Tuning.ppo_fused_step
    MAGPO_FF_FUSED_STEP=0|1     acting step of ff_ippo / ff_mappo: 1 = torso and head of both networks in one magpo_mlp_act_step launch (csrc/mlp_step.hip),
                                0 = the composed chain of dense kernels per network.  Same function, same fp32 summation order.
                                Default: see Tuning.ff_fused_step
    MAGPO_FF_SABLE_FUSED_ACT=0|1  acting step of ff_sable: 1 = encoder, value head, the A decoder iterations and the sampling in one magpo_ff_sable_act
                                launch (csrc/ff_sable_act.hip, SableGuider.act_team_fused), 0 = the kernel-by-kernel chain SableGuider.act.  Same function;
                                the one launch is the more accurate and, as measured, the slower of the two: default 0
    MAGPO_CLASS_TABLES=0        MagpoLearner: the first layers on the dense path, not on the class tables of the distinct input rows (csrc/classtab.hip,
                                DESIGN 4b); default 1 = tables wherever the environment and the network width allow them
    MAGPO_LEGACY_INIT=1         rec_magpo.learner_setup, A/B only: the torch-generator initialisation of rounds 1-3 (same distributions, other draws)
                                instead of the parameters flax creates from the net keys
"""
from __future__ import annotations

import os
from dataclasses import dataclass


@dataclass
class Tuning:
    ret_chunk_tokens: int = 0     # 0 = default (32), 32 or 64: magpo_retention_num_chunks / _chunk_fwd / _chunk_bwd
    gru_split_bf16: int = 2       # magpo_gru_scan_fwd / _bwd (2: forward scan on bf16 triples = fp32 accuracy, see above; 0: fp32 MFMA)
    gru_block_rows: int = 0       # magpo_gru_scan_fwd / _bwd / magpo_gru_carry
    linear_variant: int = 0       # magpo_linear of the guider (0, or 4 = bf16 triples for KIN 128 / 192; see include/magpo.h)
    actor_linear_variant: int = 0 # magpo_linear of the GRU actor
    wgrad_variant: int = 0        # magpo_wgrad (0, or 64 = bf16 triples for 128 x 384)
    act_envs_per_wave: int = 0    # magpo_sable_act dims[11]
    ppo_fused_step: bool = True   # critic.step_pair: magpo_gru_cell_step (True) or the composed step of each network (False)
    ff_fused_step: bool = True    # ff_nets.act_pair: magpo_mlp_act_step (True) or the composed dense chain of each network (False)
    ff_sable_fused_act: bool = False  # ff_sable acting step: SableGuider.act_team_fused / magpo_ff_sable_act (True) or the chain SableGuider.act (False)
    dense_bwd_min_rows: int = 16384   # NetBase.dense_bwd: rows from which a narrow dense layer's dW and dX come from one magpo_dense_bwd launch (64 x 256:
                                      # the size from which magpo_wgrad uses its whole-matrix kernels); below it the pair magpo_wgrad + magpo_linear.  No
                                      # environment variable: tests set the field
    class_tables: bool = True     # MagpoLearner.class_tables: first-layer class tables where env and network allow them (False: dense path)
    legacy_init: bool = False     # rec_magpo.learner_setup: the torch-generator initialisation (A/B only)

    @classmethod
    def from_env(cls, env=None) -> "Tuning":
        e = os.environ if env is None else env
        on = lambda name: e.get(name) not in (None, "") and int(e[name]) != 0
        t = cls()
        t.ret_chunk_tokens = 64 if e.get("MAGPO_RET_CHUNK") == "64" else 0
        t.gru_split_bf16 = int(e["MAGPO_GRU_SPLIT_BF16"]) if e.get("MAGPO_GRU_SPLIT_BF16") in ("0", "1", "2") else cls().gru_split_bf16
        t.gru_block_rows = int(e.get("MAGPO_GRU_BLOCK_ROWS", 0)) if e.get("MAGPO_GRU_BLOCK_ROWS") in ("32", "64") else 0
        t.linear_variant = t.actor_linear_variant = 4 if on("MAGPO_LINEAR_BF3") else 0
        t.wgrad_variant = 64 if on("MAGPO_WGRAD_BF3") else 0
        t.act_envs_per_wave = int(e["MAGPO_ACT_EPW"]) if e.get("MAGPO_ACT_EPW") in ("4", "8", "16") else 0
        t.ppo_fused_step = e["MAGPO_PPO_FUSED_STEP"] == "1" if e.get("MAGPO_PPO_FUSED_STEP") in ("0", "1") else cls().ppo_fused_step
        t.ff_fused_step = e["MAGPO_FF_FUSED_STEP"] == "1" if e.get("MAGPO_FF_FUSED_STEP") in ("0", "1") else cls().ff_fused_step
        t.ff_sable_fused_act = (e["MAGPO_FF_SABLE_FUSED_ACT"] == "1" if e.get("MAGPO_FF_SABLE_FUSED_ACT") in ("0", "1")
                                else cls().ff_sable_fused_act)
        t.class_tables = e.get("MAGPO_CLASS_TABLES", "1") != "0"
        t.legacy_init = e.get("MAGPO_LEGACY_INIT") == "1"
        return t
