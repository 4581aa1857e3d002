"""CPU reference of the fixed-grid RK4 sampler (CFM(odeint_kwargs=dict(method="rk4"))): torchdiffeq's rule restated, and CFM.sample
built around it from the oracle's public pieces.  torchdiffeq is not installed here, so the rule is an unpinned leaf, pinned by the
closed-form tests of tests/test_rk4_rule.py."""
import torch

from oracle import dit_oracle as O

_ONE_THIRD = 1 / 3
_TWO_THIRDS = 2 / 3


def rk4_odeint(fn, y0: torch.Tensor, t: torch.Tensor, keep_trajectory: bool = True):
    """torchdiffeq 0.2.5 odeint(method='rk4') on the fixed grid t: RK4._step_func -> rk4_alt_step_func, the 3/8 rule (not the classic
    1/6-1/3-1/3-1/6 one), with torchdiffeq's order of operations.  Per interval t0 = t_i, t1 = t_{i+1}, dt = t1 - t0:
        k1 = fn(t0, y);  k2 = fn(t0 + dt/3, y + dt k1 / 3);  k3 = fn(t0 + 2 dt/3, y + dt (k2 - k1/3));  k4 = fn(t1, y + dt (k1 - k2 + k3))
        y += (k1 + 3 (k2 + k3) + k4) dt / 8
    fn receives the stage times as 0-dim tensors of t's dtype."""
    ys = [y0]
    y = y0
    for i in range(t.numel() - 1):
        t0, t1 = t[i], t[i + 1]
        dt = t1 - t0
        k1 = fn(t0, y)
        k2 = fn(t0 + dt * _ONE_THIRD, y + dt * k1 * _ONE_THIRD)
        k3 = fn(t0 + dt * _TWO_THIRDS, y + dt * (k2 - k1 * _ONE_THIRD))
        k4 = fn(t1, y + dt * (k1 - k2 + k3))
        y = y + (k1 + 3 * (k2 + k3) + k4) * dt * 0.125
        if keep_trajectory:
            ys.append(y)
    if keep_trajectory:
        return torch.stack(ys)
    return y


@torch.no_grad()
def cfm_sample_rk4(sd, cfg, cond: torch.Tensor, text: torch.Tensor, duration, *, lens=None, steps=32, cfg_strength=1.0,
                   sway_sampling_coef=None, seed=None, max_duration=4096, y0=None, forward_fn=None):
    """oracle.dit_oracle.cfm_sample (CFM.sample, F/model/cfm.py:82-210) with the RK4 solver: the same setup, the same CFG-combined
    velocity `fn`, the same final overwrite of the conditioning frames.  `forward_fn` substitutes the backbone (unett_forward /
    mmdit_forward); default dit_forward.  Returns the final [b, n, mel]."""
    fwd = forward_fn or (lambda **kw: O.dit_forward(sd, cfg, **kw))
    cond = cond.float()
    b, cond_len = cond.shape[:2]
    if lens is None:
        lens = torch.full((b,), cond_len, dtype=torch.long)
    text_lens = (text != -1).sum(dim=-1)
    lens = torch.maximum(text_lens, lens)
    cond_mask = O.lens_to_mask(lens)
    if isinstance(duration, int):
        duration = torch.full((b,), duration, dtype=torch.long)
    duration = torch.maximum(lens + 1, duration).clamp(max=max_duration)
    nmax = int(duration.amax())
    cond = torch.nn.functional.pad(cond, (0, 0, 0, nmax - cond_len), value=0.0)
    cond_mask = torch.nn.functional.pad(cond_mask, (0, nmax - cond_mask.shape[-1]), value=False)[..., None]
    step_cond = torch.where(cond_mask, cond, torch.zeros_like(cond))
    mask = O.lens_to_mask(duration) if b > 1 else None

    def fn(t, x):
        pred = fwd(x=x, cond=step_cond, text=text, time=t, mask=mask, drop_audio_cond=False, drop_text=False)
        if cfg_strength < 1e-5:
            return pred
        null = fwd(x=x, cond=step_cond, text=text, time=t, mask=mask, drop_audio_cond=True, drop_text=True)
        return pred + (pred - null) * cfg_strength

    y0 = O.make_noise(duration, cfg.mel_dim, seed, y0)
    t = O.sway_time_grid(steps, sway_sampling_coef)
    last = rk4_odeint(fn, y0, t, keep_trajectory=False)
    return torch.where(cond_mask, cond, last)
