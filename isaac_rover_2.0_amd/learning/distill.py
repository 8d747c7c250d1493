"""Distilling a teacher into the recurrent student — the last step of the reference's learning-by-cheating scheme, on the MI355X.

The reference ships the student (``tasks/utils/learning_by_cheating/student_model.py``) but no training loop, so the loss is THIS
project's definition (tests/student_grad_ref.py restates it in float64):

    L = mean over B, T, A of (actions - teacher_actions)^2  +  recon_scale * mean over B, T, S + D of (estimated - target)^2

``actions`` and ``estimated`` are ``StudentPolicy.forward_train``'s over a window x [B, T, F]; ``target`` defaults to the window's own
sparse | dense columns (pass the clean heightmaps when the student's are noised).  The two gradients at the outputs,
``2 (a - a*) / (B T A)`` and ``2 recon_scale (e - e*) / (B T (S + D))``, and the reported loss values are elementwise torch; everything
behind them is ``StudentPolicy.backward`` (back-propagation through time on the HIP kernels) and one optimiser step over the student's
trainable tensors: ``learning/optim.py``'s ``Adam`` (``rover_optim_step``: clip + Adam in two launches) or, with ``native_step=False``,
``torch.nn.utils.clip_grad_norm_`` + ``torch.optim.Adam`` as ``PPO`` offers.  Nothing here synchronises.

Windows of one rollout are chained by the hidden state (truncated back-propagation through time): ``update()`` returns the state
after the window, computed with the parameters BEFORE the step; hand it back as the next window's ``h0``.
"""
from __future__ import annotations

import torch

from .optim import Adam


class StudentTrainer:
    def __init__(self, engine, student, lr=1e-4, grad_norm_clip=1.0, recon_scale=0.5, native_step=True):
        if not lr >= 0.0:
            raise ValueError(f"StudentTrainer: lr = {lr}")
        if not recon_scale >= 0.0:
            raise ValueError(f"StudentTrainer: recon_scale = {recon_scale}")
        if not grad_norm_clip >= 0.0:
            raise ValueError(f"StudentTrainer: grad_norm_clip = {grad_norm_clip} (0: no clipping)")
        self.engine, self.student = engine, student
        self.grad_norm_clip, self.recon_scale, self.native_step = float(grad_norm_clip), float(recon_scale), bool(native_step)
        self.params = student.parameters()
        for p in self.params:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        self.optimizer = Adam(engine, self.params, lr=float(lr)) if self.native_step else torch.optim.Adam(self.params, lr=float(lr))

    def loss_and_grads(self, x, teacher_actions, h0=None, reset=None, target=None):
        """One window forward and back: x [B, T, F], teacher_actions [B, T, A], h0 [n_layers, B, H] (None: zeros), reset [B, T] (None:
        no episode boundary), target [B, T, S + D] (None: x's own heightmap columns) -> (loss, action_loss, recon_loss) as device
        scalars.  Leaves the gradients in the parameters' ``.grad``, the gradient at h0 in ``self.dh0`` and the state after the window
        in ``self.h``."""
        st = self.student
        if x is None or x.dim() != 3:
            raise ValueError("StudentTrainer: x must be [B, T, F]")
        b, t_len, f = x.shape
        na, ex = st.info["actions"], st.info["sparse"] + st.info["dense"]
        if teacher_actions is None or tuple(teacher_actions.shape) != (b, t_len, na):
            raise ValueError(f"StudentTrainer: teacher_actions must be [{b}, {t_len}, {na}]")
        if target is not None and tuple(target.shape) != (b, t_len, ex):
            raise ValueError(f"StudentTrainer: target must be [{b}, {t_len}, {ex}]")
        if h0 is None:
            h0 = torch.zeros(st.n_layers, b, st.hidden_dim, device=x.device)
        actions, est, self.h = st.forward_train(x, h0, reset)
        if target is None:
            target = x[:, :, f - ex:]
        da, de = actions - teacher_actions, est - target
        action_loss, recon_loss = (da * da).mean(), (de * de).mean()
        d_actions = da * (2.0 / da.numel())
        d_est = de * (2.0 * self.recon_scale / de.numel()) if self.recon_scale > 0.0 and ex > 0 else None
        self.dh0 = st.backward(d_actions, d_est)
        return action_loss + self.recon_scale * recon_loss, action_loss, recon_loss

    def step(self):
        """Gradient-norm clip and one Adam step on the gradients in ``.grad``."""
        if self.native_step:
            self.optimizer.step(self.grad_norm_clip)
            return
        if self.grad_norm_clip > 0:
            torch.nn.utils.clip_grad_norm_(self.params, self.grad_norm_clip)
        self.optimizer.step()

    def update(self, x, teacher_actions, h0=None, reset=None, target=None):
        """``loss_and_grads`` and one optimiser step -> (loss, action_loss, recon_loss, h): the three losses of the window BEFORE the
        step, and the hidden state after the window [n_layers, B, H] — the next window's ``h0``."""
        losses = self.loss_and_grads(x, teacher_actions, h0, reset, target)
        self.step()
        return losses + (self.h,)
