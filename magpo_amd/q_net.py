"""Recurrent Q network (RecQNetwork, mava/networks/base.py:229-273) on the MI355X kernels.

pre-torso -> scanned GRU(128) with resets -> post-torso -> Dense(num_actions, orthogonal(0.01)): the shape of ``GruActor`` with its logit rows
read as Q rows, so parameter layout, initialisation from a key, ``seq_fwd`` / ``seq_bwd``, ``load_named`` and ``refresh`` are the actor's.
``step`` runs the GRU cell through one ``magpo_gru_cell_step`` launch (nnets = 1).  The torsos follow ``network.q_network.{pre,post}_torso``.
"""
from __future__ import annotations

from .actor import GruActor
from .critic import gru_cell_step


class GruQNetwork(GruActor):
    def step(self, obs, h_in, reset_env, h_out, want_logits: bool = True):
        """One step for N envs: obs [N, A, F], h_in / h_out [N * A, 128], reset_env [N] u8 (term_or_trunc of the previous step).  Returns the
        Q rows [N * A, 64] (K valid columns; a workspace of this object), or None without ``want_logits``."""
        R = obs.shape[0] * self.A
        emb = self.pre_torso(obs, self.Fld, R, "s_")[-1][3]
        gru_cell_step((self,), (emb,), (h_in,), reset_env, (h_out,), self.A)
        if not want_logits:
            return None
        q = self.b.get("s_logits", (R, 64), zero=True)
        self.post_torso_logits(h_out, R, "s_", q)
        return q


GruQNetwork.apply = GruQNetwork.seq_fwd   # q_net.apply(..., method="get_q_values") (rec_iql.py:310): the scanned training forward
