"""Samplers (k-diffusion style, sigma space).

The reference's users pick these by name (its sampler-speed table
worker.py:75-94 lists what people run); implemented natively: Euler,
Euler a, DDIM (= Euler on the discrete schedule), DDPM, Heun, LMS,
DPM2/DPM2 a, DPM++ 2M / SDE / 2S a / 2M SDE / 3M SDE, UniPC, LCM and
Restart, each verified against a point-mass oracle (the update algebra
must land exactly on x0 with an exact denoiser). Per-step state updates
are fused elementwise HIP kernels on GPU (ops.euler_step /
ops.add_noise / ops.lincomb) so the denoise loop is hipGraph-capturable.

model_fn(x_scaled, t) -> eps; the driver loop in pipeline.py owns CFG,
interrupts and callbacks.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional

import torch

from .. import ops
from .schedule import Schedule

ModelFn = Callable[[torch.Tensor, float], torch.Tensor]
StepCallback = Optional[Callable[[int, int], None]]


def _denoised(x: torch.Tensor, eps: torch.Tensor, sigma: float) -> torch.Tensor:
    return ops.lincomb(x, eps, 1.0, -sigma)


def _eval(model_fn: ModelFn, x: torch.Tensor, sigma: float, t: float):
    """Scale input to unit variance, call the eps-model, return denoised."""
    c_in = 1.0 / math.sqrt(sigma * sigma + 1.0)
    eps = model_fn(ops.scale(x, c_in), t)
    return _denoised(x, eps, sigma)


def _noised(x: torch.Tensor, noise_fn, amp: float) -> torch.Tensor:
    """x + amp * (the next draw of noise_fn). A noise source with add_to
    (pipeline/noise.py) fuses the draw into the update; a plain callable
    returning the noise tensor works as before."""
    add_to = getattr(noise_fn, "add_to", None)
    if add_to is not None:
        return add_to(x, 1.0, amp)
    return ops.add_noise(x, noise_fn(), 1.0, amp)


def _ancestral_sigmas(sigma: float, sigma_next: float, eta: float = 1.0):
    if sigma_next <= 0:
        return 0.0, 0.0
    su = min(
        sigma_next,
        eta
        * math.sqrt(
            sigma_next**2 * (sigma**2 - sigma_next**2) / (sigma**2)
        ),
    )
    sd = math.sqrt(sigma_next**2 - su**2)
    return sd, su


class Sampler:
    """Base: walks the schedule, delegates the per-step update."""

    order = 1  # model evals per step
    # sdwui "Eta" (ancestral-noise multiplier, opts eta_ancestral /
    # eta_ddim): consumed by the ancestral and SDE families; 0 makes
    # them deterministic. Overridden per request via the API `eta` field.
    eta = 1.0

    def __init__(self, schedule: Schedule):
        self.schedule = schedule
        # k-diffusion stochasticity knobs (sdwui s_churn/s_tmin/s_tmax/
        # s_noise); honored by the Euler/Heun family via _churned
        self.s_churn = 0.0
        self.s_tmin = 0.0
        self.s_tmax = float("inf")
        self.s_noise = 1.0

    def _churned(self, x, sigma, noise_fn):
        """Temporarily raise sigma by gamma (k-diffusion churn); returns
        (x_hat, sigma_hat)."""
        if self.s_churn <= 0 or not (self.s_tmin <= sigma <= self.s_tmax):
            return x, sigma
        gamma = min(
            self.s_churn / max(1, self.schedule.steps), 2 ** 0.5 - 1
        )
        sigma_hat = sigma * (1 + gamma)
        if noise_fn is not None and sigma_hat > sigma:
            extra = (sigma_hat ** 2 - sigma ** 2) ** 0.5 * self.s_noise
            x = _noised(x, noise_fn, extra)
        return x, sigma_hat

    def sample(
        self,
        model_fn: ModelFn,
        x: torch.Tensor,
        noise_fn: Optional[Callable[[], torch.Tensor]] = None,
        callback: StepCallback = None,
        interrupt: Optional[Callable[[], bool]] = None,
        post_step: Optional[Callable[[torch.Tensor, float], torch.Tensor]] = None,
    ) -> torch.Tensor:
        """post_step(x, sigma_next) transforms the state after each update
        (inpainting re-imposes the init outside the mask there)."""
        sig = self.schedule.sigmas.tolist()
        ts = self.schedule.timesteps.tolist()
        self.reset()
        for i in range(len(ts)):
            if interrupt is not None and interrupt():
                break
            t_next = ts[i + 1] if i + 1 < len(ts) else ts[i]
            x = self.step(
                model_fn, x, sig[i], sig[i + 1], ts[i], noise_fn, t_next
            )
            if post_step is not None:
                x = post_step(x, sig[i + 1])
            if callback is not None:
                callback(i + 1, len(ts))
        return x

    def reset(self) -> None:
        pass

    def step(self, model_fn, x, sigma, sigma_next, t, noise_fn,
             t_next=None):
        raise NotImplementedError

    @staticmethod
    def _t_for(sigma_mid, sigma, sigma_next, t, t_next):
        """Interpolate the train-timestep for an intermediate sigma
        (log-sigma linear, matching the schedule construction)."""
        if sigma_next <= 0 or t_next is None or t_next == t:
            return t
        w = (math.log(sigma_mid) - math.log(sigma)) / (
            math.log(sigma_next) - math.log(sigma)
        )
        return t + w * (t_next - t)


class Euler(Sampler):
    def step(self, model_fn, x, sigma, sigma_next, t, noise_fn,
             t_next=None):
        x, sigma = self._churned(x, sigma, noise_fn)
        denoised = _eval(model_fn, x, sigma, t)
        return ops.euler_step(x, denoised, sigma, sigma_next)


class EulerAncestral(Sampler):
    def step(self, model_fn, x, sigma, sigma_next, t, noise_fn,
             t_next=None):
        denoised = _eval(model_fn, x, sigma, t)
        if self.eta == 0:
            # deterministic path is bit-exact Euler (no sqrt round trip)
            return ops.euler_step(x, denoised, sigma, sigma_next)
        sd, su = _ancestral_sigmas(sigma, sigma_next, self.eta)
        x = ops.euler_step(x, denoised, sigma, sd)
        if su > 0 and noise_fn is not None:
            x = _noised(x, noise_fn, su)
        return x


class DDIMSampler(EulerAncestral):
    """Deterministic DDIM == Euler in sigma space (eta 0, sdwui's
    eta_ddim default); a request-level eta > 0 restores the stochastic
    DDIM update (ancestral noise scaled by eta)."""

    eta = 0.0


class Heun(Sampler):
    order = 2

    def step(self, model_fn, x, sigma, sigma_next, t, noise_fn,
             t_next=None):
        x, sigma = self._churned(x, sigma, noise_fn)
        denoised = _eval(model_fn, x, sigma, t)
        if sigma_next <= 0:
            return ops.euler_step(x, denoised, sigma, sigma_next)
        x1 = ops.euler_step(x, denoised, sigma, sigma_next)
        denoised2 = _eval(model_fn, x1, sigma_next, t)
        d1 = ops.lincomb(x, denoised, 1.0 / sigma, -1.0 / sigma)
        d2 = ops.lincomb(x1, denoised2, 1.0 / sigma_next, -1.0 / sigma_next)
        d = ops.lincomb(d1, d2, 0.5, 0.5)
        return ops.lincomb(x, d, 1.0, sigma_next - sigma)


class DPMpp2M(Sampler):
    def reset(self):
        self.old_denoised = None
        self.h_last = None

    def step(self, model_fn, x, sigma, sigma_next, t, noise_fn,
             t_next=None):
        denoised = _eval(model_fn, x, sigma, t)
        tt = -math.log(sigma)
        if sigma_next <= 0:
            self.old_denoised = denoised
            return denoised
        tn = -math.log(sigma_next)
        h = tn - tt
        if self.old_denoised is None or self.h_last is None:
            d = denoised
        else:
            r = self.h_last / h
            d = ops.lincomb(
                denoised, self.old_denoised, 1 + 1 / (2 * r), -1 / (2 * r)
            )
        x = ops.lincomb(x, d, sigma_next / sigma, -math.expm1(-h))
        self.old_denoised = denoised
        self.h_last = h
        return x


class DPMppSDE(Sampler):
    """DPM++ SDE (2-eval, ancestral-noise) — simplified 2S form."""

    order = 2

    def step(self, model_fn, x, sigma, sigma_next, t, noise_fn,
             t_next=None):
        denoised = _eval(model_fn, x, sigma, t)
        if sigma_next <= 0:
            return denoised
        # midpoint in log-sigma
        sigma_mid = math.exp((math.log(sigma) + math.log(sigma_next)) / 2)
        x_mid = ops.euler_step(x, denoised, sigma, sigma_mid)
        t_mid = self._t_for(sigma_mid, sigma, sigma_next, t, t_next)
        denoised2 = _eval(model_fn, x_mid, sigma_mid, t_mid)
        sd, su = _ancestral_sigmas(sigma, sigma_next, self.eta)
        x = ops.euler_step(x, denoised2, sigma, sd)
        if su > 0 and noise_fn is not None:
            x = _noised(x, noise_fn, su)
        return x


class DPMpp2MSDE(Sampler):
    """DPM++ 2M SDE (k-diffusion sample_dpmpp_2m_sde, midpoint solver,
    eta=1): the 2M multistep update with an SDE noise injection."""

    eta = 1.0

    def reset(self):
        self.old_denoised = None
        self.h_last = None

    def step(self, model_fn, x, sigma, sigma_next, t, noise_fn,
             t_next=None):
        denoised = _eval(model_fn, x, sigma, t)
        if sigma_next <= 0:
            self.old_denoised = denoised
            return denoised
        tt, tn = -math.log(sigma), -math.log(sigma_next)
        h = tn - tt
        eta_h = self.eta * h
        decay = math.exp(-eta_h)
        phi = -math.expm1(-h - eta_h)
        x = ops.lincomb(x, denoised, (sigma_next / sigma) * decay, phi)
        if self.old_denoised is not None and self.h_last is not None:
            r = self.h_last / h
            d = ops.lincomb(denoised, self.old_denoised, 1.0, -1.0)
            x = ops.lincomb(x, d, 1.0, self._ms_coeff(phi, h, eta_h) / r)
        if self.eta > 0 and noise_fn is not None:
            amp = sigma_next * math.sqrt(max(0.0, -math.expm1(-2 * eta_h)))
            x = _noised(x, noise_fn, amp)
        self.old_denoised = denoised
        self.h_last = h
        return x

    @staticmethod
    def _ms_coeff(phi: float, h: float, eta_h: float) -> float:
        # midpoint solver: half the decayed step weight
        return 0.5 * phi


class DPMpp2MSDEHeun(DPMpp2MSDE):
    """DPM++ 2M SDE with the Heun ('improved Euler') solver: the
    multistep difference term carries the exact second-order weight
    phi_2 = 1 - phi/(h + eta*h) instead of the midpoint 0.5*phi; both
    agree to O(h) as h -> 0 (phi ~ h + ...) and share the decay/noise
    schedule. sdwui's 'DPM++ 2M SDE Heun' sampler family."""

    @staticmethod
    def _ms_coeff(phi: float, h: float, eta_h: float) -> float:
        return 1.0 - phi / (h + eta_h)


class DPMpp3MSDE(Sampler):
    """DPM++ 3M SDE (k-diffusion sample_dpmpp_3m_sde, eta=1): third-order
    multistep with SDE noise."""

    eta = 1.0

    def reset(self):
        self.den_1 = None
        self.den_2 = None
        self.h_1 = None
        self.h_2 = None

    def step(self, model_fn, x, sigma, sigma_next, t, noise_fn,
             t_next=None):
        denoised = _eval(model_fn, x, sigma, t)
        if sigma_next <= 0:
            return denoised
        tt, tn = -math.log(sigma), -math.log(sigma_next)
        h = tn - tt
        h_eta = h * (self.eta + 1.0)
        phi_1 = -math.expm1(-h_eta)
        x = ops.lincomb(x, denoised, math.exp(-h_eta), phi_1)
        if self.den_1 is not None and self.h_1 is not None:
            phi_2 = phi_1 / h_eta - 1.0  # note: negative of k-diff's phi_2
            if self.den_2 is not None and self.h_2 is not None:
                r0, r1 = self.h_1 / h, self.h_2 / h
                d1_0 = ops.lincomb(denoised, self.den_1, 1 / r0, -1 / r0)
                d1_1 = ops.lincomb(self.den_1, self.den_2, 1 / r1, -1 / r1)
                d1 = ops.lincomb(
                    d1_0, ops.lincomb(d1_0, d1_1, 1.0, -1.0),
                    1.0, r0 / (r0 + r1),
                )
                d2 = ops.lincomb(
                    d1_0, d1_1, 1 / (r0 + r1), -1 / (r0 + r1)
                )
                # k-diff: x += phi2_kd*d1 - phi3_kd*d2 with
                # phi2_kd = -phi_2, phi3_kd = phi2_kd/h_eta - 0.5
                phi_3 = phi_2 / h_eta + 0.5  # = -phi3_kd
                x = ops.lincomb(x, d1, 1.0, -phi_2)
                x = ops.lincomb(x, d2, 1.0, phi_3)
            else:
                r = self.h_1 / h
                d = ops.lincomb(denoised, self.den_1, 1 / r, -1 / r)
                x = ops.lincomb(x, d, 1.0, -phi_2)
        if self.eta > 0 and noise_fn is not None:
            amp = sigma_next * math.sqrt(
                max(0.0, -math.expm1(-2 * h * self.eta))
            )
            x = _noised(x, noise_fn, amp)
        self.den_2 = self.den_1
        self.den_1 = denoised
        self.h_2 = self.h_1
        self.h_1 = h
        return x


class DPM2(Sampler):
    """k-diffusion sample_dpm_2: explicit midpoint in log-sigma."""

    order = 2
    eta = 0.0

    def step(self, model_fn, x, sigma, sigma_next, t, noise_fn,
             t_next=None):
        denoised = _eval(model_fn, x, sigma, t)
        sd, su = _ancestral_sigmas(sigma, sigma_next, self.eta)
        if sd <= 0:
            return ops.euler_step(x, denoised, sigma, sigma_next)
        sigma_mid = math.exp((math.log(sigma) + math.log(sd)) / 2)
        x_mid = ops.euler_step(x, denoised, sigma, sigma_mid)
        t_mid = self._t_for(sigma_mid, sigma, sigma_next, t, t_next)
        denoised2 = _eval(model_fn, x_mid, sigma_mid, t_mid)
        # full step from sigma with the midpoint derivative:
        # x + d2 * (sd - sigma), d2 = (x_mid - denoised2) / sigma_mid
        d2 = ops.lincomb(x_mid, denoised2, 1.0 / sigma_mid, -1.0 / sigma_mid)
        x = ops.lincomb(x, d2, 1.0, sd - sigma)
        if su > 0 and noise_fn is not None:
            x = _noised(x, noise_fn, su)
        return x


class DPM2Ancestral(DPM2):
    eta = 1.0


class DPMpp2SAncestral(Sampler):
    """DPM++ 2S a (k-diffusion sample_dpmpp_2s_ancestral): single-step
    second-order update to the ancestral down-sigma, then ancestral noise."""

    order = 2

    def step(self, model_fn, x, sigma, sigma_next, t, noise_fn,
             t_next=None):
        denoised = _eval(model_fn, x, sigma, t)
        if sigma_next <= 0:
            return denoised
        sd, su = _ancestral_sigmas(sigma, sigma_next, self.eta)
        tt, tn = -math.log(sigma), -math.log(sd)
        h = tn - tt
        s = tt + 0.5 * h
        sig_s = math.exp(-s)
        x2 = ops.lincomb(
            x, denoised, sig_s / sigma, -math.expm1(-(s - tt))
        )
        t_mid = self._t_for(sig_s, sigma, sigma_next, t, t_next)
        denoised2 = _eval(model_fn, x2, sig_s, t_mid)
        x = ops.lincomb(x, denoised2, sd / sigma, -math.expm1(-h))
        if su > 0 and noise_fn is not None:
            x = _noised(x, noise_fn, su)
        return x


class UniPC(Sampler):
    """UniPC (bh2 variant, data prediction, order <= 3) in sigma space.

    Predictor-corrector multistep: the corrector's model evaluation at the
    new point is cached and reused as the next step's predictor evaluation,
    so the amortized cost is one model eval per step — the same trick the
    original uni_pc sampling loop uses.
    """

    max_order = 3

    def reset(self):
        self.m: List[torch.Tensor] = []  # x0 predictions, newest last
        self.lam: List[float] = []
        self._pending = None  # (x tensor, model eval) from the corrector

    def _rhos(self, h: float, rks: List[float]):
        """bh2 coefficients: solve R rhos = b (R[k][i] = rks[i]**k)."""
        hh = -h
        h_phi_1 = math.expm1(hh)
        b_h = h_phi_1  # bh2: B(h) = expm1(hh)
        b = []
        h_phi_k = h_phi_1 / hh - 1
        for k in range(1, len(rks) + 1):
            b.append(h_phi_k * math.factorial(k) / b_h)
            h_phi_k = h_phi_k / hh - 1 / math.factorial(k + 1)
        n = len(rks)
        if n == 1:
            return [b[0]], h_phi_1, b_h
        import numpy as np

        R = np.array([[r ** k for r in rks] for k in range(n)])
        rhos = np.linalg.solve(R, np.array(b))
        return [float(v) for v in rhos], h_phi_1, b_h

    def step(self, model_fn, x, sigma, sigma_next, t, noise_fn,
             t_next=None):
        if self._pending is not None and self._pending[0] is x:
            m0 = self._pending[1]  # corrector eval from the previous step
        else:
            m0 = _eval(model_fn, x, sigma, t)
        self._pending = None
        lam0 = -math.log(sigma)
        self.m.append(m0)
        self.lam.append(lam0)
        if len(self.m) > self.max_order:
            self.m.pop(0)
            self.lam.pop(0)
        if sigma_next <= 0:
            return m0
        lam_t = -math.log(sigma_next)
        h = lam_t - lam0
        order = min(len(self.m), self.max_order)
        # history ratios and differences (newest-first back through history)
        rks = [
            (self.lam[-1 - k] - lam0) / h for k in range(1, order)
        ]
        d1s = [
            ops.lincomb(self.m[-1 - k], m0, 1.0 / rks[k - 1], -1.0 / rks[k - 1])
            for k in range(1, order)
        ]
        # predictor
        base = ops.lincomb(x, m0, sigma_next / sigma, -math.expm1(-h))
        if rks:
            rhos_p, _, b_h = self._rhos(h, rks)
            x_t = base
            for r, d in zip(rhos_p, d1s):
                x_t = ops.lincomb(x_t, d, 1.0, -b_h * r)
        else:
            x_t = base
        # corrector (skipped at sigma 0, handled above)
        m_t = _eval(
            model_fn, x_t, sigma_next, t_next if t_next is not None else t
        )
        rhos_c, _, b_h = self._rhos(h, rks + [1.0])
        x_c = base
        for r, d in zip(rhos_c[:-1], d1s):
            x_c = ops.lincomb(x_c, d, 1.0, -b_h * r)
        d1_t = ops.lincomb(m_t, m0, 1.0, -1.0)
        x_c = ops.lincomb(x_c, d1_t, 1.0, -b_h * rhos_c[-1])
        self._pending = (x_c, m_t)
        return x_c


class Restart(Sampler):
    """Restart sampling (Xu et al. 2023; the shape of sdwui's 'Restart'):
    Heun descent plus K re-noise restarts across a mid-sigma band —
    re-injecting noise and re-descending contracts accumulated error.

    Simplified parameterization: band = sigmas within [0.1, 2.0] on the
    existing schedule, K = 2 restart cycles (sdwui derives the band from a
    separate Karras sub-schedule; the mechanism and cost profile match).
    """

    order = 2  # Heun-style double eval per step, plus restart overhead

    K_RESTART = 2
    BAND_HI = 2.0
    BAND_LO = 0.1

    def sample(self, model_fn, x, noise_fn=None, callback=None,
               interrupt=None, post_step=None):
        heun = Heun(self.schedule)
        heun.s_churn = self.s_churn
        heun.s_tmin = self.s_tmin
        heun.s_tmax = self.s_tmax
        heun.s_noise = self.s_noise
        sig = self.schedule.sigmas.tolist()
        ts = self.schedule.timesteps.tolist()
        n = len(ts)
        # band indices on the schedule
        a = next((i for i in range(n) if sig[i] <= self.BAND_HI), 0)
        bi = next((i for i in range(n) if sig[i] <= self.BAND_LO), n)
        restarts = self.K_RESTART if 0 <= a < bi <= n and bi - a >= 2 else 0
        total = n + restarts * (bi - a)
        done = 0

        def descend(x, i0, i1):
            nonlocal done
            for i in range(i0, i1):
                if interrupt is not None and interrupt():
                    return x, True
                t_next = ts[i + 1] if i + 1 < n else ts[i]
                x = heun.step(
                    model_fn, x, sig[i], sig[i + 1], ts[i], noise_fn, t_next
                )
                if post_step is not None:
                    x = post_step(x, sig[i + 1])
                done += 1
                if callback is not None:
                    callback(min(done, total), total)
            return x, False

        x, stop = descend(x, 0, bi)
        if not stop and restarts and noise_fn is not None:
            s_hi, s_lo = sig[a], sig[bi]
            for _ in range(restarts):
                bump = math.sqrt(max(0.0, s_hi * s_hi - s_lo * s_lo))
                x = _noised(x, noise_fn, bump)
                x, stop = descend(x, a, bi)
                if stop:
                    break
        if not stop:
            x, stop = descend(x, bi, n)
        return x


class LCM(Sampler):
    """Latent-consistency sampling: jump straight to the denoised estimate,
    then re-noise to the next sigma (sdwui's LCM sampler shape)."""

    def step(self, model_fn, x, sigma, sigma_next, t, noise_fn,
             t_next=None):
        denoised = _eval(model_fn, x, sigma, t)
        if sigma_next <= 0 or noise_fn is None:
            return denoised
        return _noised(denoised, noise_fn, sigma_next)


class _DPMSolver(Sampler):
    """Shared DPM-Solver (Lu et al. 2022) machinery in t = -log(sigma)
    space, eps-model form (k-diffusion DPMSolver). The fast/adaptive
    samplers below run their own t-grids, so sigma -> train-timestep goes
    through the full sigma table rather than the step schedule."""

    def __init__(self, schedule: Schedule):
        super().__init__(schedule)
        from .schedule import make_sigmas_full

        self._table = make_sigmas_full()

    def _tt(self, sigma: float) -> float:
        from .schedule import _timesteps_for

        return float(
            _timesteps_for(torch.tensor([float(sigma)]), self._table)[0]
        )

    def _eps(self, model_fn, x, sigma: float):
        den = _eval(model_fn, x, sigma, self._tt(sigma))
        return ops.lincomb(x, den, 1.0 / sigma, -1.0 / sigma)

    @staticmethod
    def _sig(t: float) -> float:
        return math.exp(-t)

    def _step1(self, model_fn, x, t, tn, eps=None):
        h = tn - t
        if eps is None:
            eps = self._eps(model_fn, x, self._sig(t))
        return ops.lincomb(x, eps, 1.0, -self._sig(tn) * math.expm1(h)), eps

    def _step2(self, model_fn, x, t, tn, eps=None, r1=0.5):
        h = tn - t
        if eps is None:
            eps = self._eps(model_fn, x, self._sig(t))
        s1 = t + r1 * h
        u1 = ops.lincomb(
            x, eps, 1.0, -self._sig(s1) * math.expm1(r1 * h)
        )
        eps_r1 = self._eps(model_fn, u1, self._sig(s1))
        x2 = ops.lincomb(x, eps, 1.0, -self._sig(tn) * math.expm1(h))
        d = ops.lincomb(eps_r1, eps, 1.0, -1.0)
        x2 = ops.lincomb(
            x2, d, 1.0, -self._sig(tn) / (2 * r1) * math.expm1(h)
        )
        return x2, eps

    def _step3(self, model_fn, x, t, tn, eps=None, r1=1.0 / 3, r2=2.0 / 3):
        h = tn - t
        if eps is None:
            eps = self._eps(model_fn, x, self._sig(t))
        s1, s2 = t + r1 * h, t + r2 * h
        u1 = ops.lincomb(
            x, eps, 1.0, -self._sig(s1) * math.expm1(r1 * h)
        )
        eps_r1 = self._eps(model_fn, u1, self._sig(s1))
        u2 = ops.lincomb(
            x, eps, 1.0, -self._sig(s2) * math.expm1(r2 * h)
        )
        d1 = ops.lincomb(eps_r1, eps, 1.0, -1.0)
        u2 = ops.lincomb(
            u2, d1, 1.0,
            -self._sig(s2) * (r2 / r1)
            * (math.expm1(r2 * h) / (r2 * h) - 1.0),
        )
        eps_r2 = self._eps(model_fn, u2, self._sig(s2))
        x3 = ops.lincomb(x, eps, 1.0, -self._sig(tn) * math.expm1(h))
        d2 = ops.lincomb(eps_r2, eps, 1.0, -1.0)
        x3 = ops.lincomb(
            x3, d2, 1.0, -self._sig(tn) / r2 * (math.expm1(h) / h - 1.0)
        )
        return x3, eps


class DPMFast(_DPMSolver):
    """k-diffusion sample_dpm_fast: a fixed model-eval budget spent on a
    uniform t-grid of mixed 3rd/2nd/1st-order DPM-Solver steps (the
    reference's sampler-speed table lists it at +15.5% vs Euler a)."""

    def sample(self, model_fn, x, noise_fn=None, callback=None,
               interrupt=None, post_step=None):
        sig = self.schedule.sigmas.tolist()
        smax = sig[0]
        smin = next(s for s in reversed(sig) if s > 0)
        nfe = max(2, len(sig) - 1)
        t0, t1 = -math.log(smax), -math.log(smin)
        m = nfe // 3 + 1
        ts = [t0 + (t1 - t0) * i / m for i in range(m + 1)]
        if nfe % 3 == 0:
            orders = [3] * (m - 2) + [2, 1]
        else:
            orders = [3] * (m - 1) + [nfe % 3]
        steps = {1: self._step1, 2: self._step2, 3: self._step3}
        for i in range(m):
            if interrupt is not None and interrupt():
                return x
            x, _ = steps[orders[i]](model_fn, x, ts[i], ts[i + 1])
            if post_step is not None:
                x = post_step(x, self._sig(ts[i + 1]))
            if callback is not None:
                callback(i + 1, m)
        return x


class DPMAdaptive(_DPMSolver):
    """k-diffusion sample_dpm_adaptive (order 3, I-controller defaults):
    embedded 2nd/3rd-order error estimate drives the step size; the model
    eval count is error-controlled, not the requested step count (the
    reference's table lists it at -61% vs Euler a, i.e. ~2.5x the evals)."""

    RTOL, ATOL = 0.05, 0.0078
    H_INIT = 0.05
    ACCEPT_SAFETY = 0.81
    MAX_EVALS_FACTOR = 12  # runaway bound

    def sample(self, model_fn, x, noise_fn=None, callback=None,
               interrupt=None, post_step=None):
        sig = self.schedule.sigmas.tolist()
        smax = sig[0]
        smin = next(s for s in reversed(sig) if s > 0)
        t_end = -math.log(smin)
        s_cur = -math.log(smax)
        h = self.H_INIT
        errs: list = []
        x_prev = x
        nominal = max(1, self.schedule.steps)
        max_evals = self.MAX_EVALS_FACTOR * nominal
        evals = done = 0
        while s_cur < t_end - 1e-5 and evals < max_evals:
            if interrupt is not None and interrupt():
                return x
            t = min(t_end, s_cur + h)
            x_low, eps = self._step2(model_fn, x, s_cur, t, r1=1.0 / 3)
            x_high, _ = self._step3(model_fn, x, s_cur, t, eps=eps)
            evals += 5
            delta = torch.maximum(
                torch.full_like(x_low, self.ATOL),
                self.RTOL
                * torch.maximum(x_low.float().abs(), x_prev.float().abs()),
            )
            err = float(
                torch.linalg.vector_norm(
                    (x_low.float() - x_high.float()) / delta
                )
                / x_low.numel() ** 0.5
            )
            inv_err = 1.0 / (err + 1e-8)
            if not errs:
                errs = [inv_err] * 3
            errs[0] = inv_err
            factor = 1.0 + math.atan(errs[0] ** (1.0 / 3.0) - 1.0)
            accept = factor >= self.ACCEPT_SAFETY
            h *= factor
            if accept:
                errs[2], errs[1] = errs[1], errs[0]
                x_prev = x_low
                x = x_high
                s_cur = t
                if post_step is not None:
                    x = post_step(x, self._sig(s_cur))
                done += 1
                if callback is not None:
                    callback(min(done, nominal), nominal)
        if callback is not None:
            callback(nominal, nominal)
        return x


class LMS(Sampler):
    """Linear multistep (order <= 4) with exactly integrated Adams
    coefficients over each sigma interval (k-diffusion sample_lms)."""

    max_order = 4

    def reset(self):
        self.ds: List[torch.Tensor] = []
        self.step_idx = 0

    def _coeff(self, order, j, sigmas, i):
        from scipy import integrate

        def fn(tau):
            prod = 1.0
            for k in range(order):
                if j == k:
                    continue
                prod *= (tau - sigmas[i - k]) / (sigmas[i - j] - sigmas[i - k])
            return prod

        val, _ = integrate.quad(fn, sigmas[i], sigmas[i + 1], epsrel=1e-4)
        return val

    def step(self, model_fn, x, sigma, sigma_next, t, noise_fn,
             t_next=None):
        denoised = _eval(model_fn, x, sigma, t)
        d = ops.lincomb(x, denoised, 1.0 / sigma, -1.0 / sigma)
        self.ds.append(d)
        if len(self.ds) > self.max_order:
            self.ds.pop(0)
        sigmas = self.schedule.sigmas.tolist()
        i = self.step_idx
        order = min(i + 1, self.max_order)
        coeffs = [self._coeff(order, j, sigmas, i) for j in range(order)]
        out = x.float()
        for c, dj in zip(coeffs, reversed(self.ds)):
            out = out + c * dj.float()
        self.step_idx += 1
        return out.to(x.dtype)


SAMPLERS: Dict[str, type] = {
    "Euler": Euler,
    "Euler a": EulerAncestral,
    "DDIM": DDIMSampler,  # eta 0 == Euler in sigma space; eta>0 noises
    "Heun": Heun,
    "DPM++ 2M": DPMpp2M,
    "DPM++ 2M Karras": DPMpp2M,
    "DPM++ SDE": DPMppSDE,
    "DPM++ SDE Karras": DPMppSDE,
    "DPM++ 2M SDE": DPMpp2MSDE,
    "DPM++ 2M SDE Karras": DPMpp2MSDE,
    "DPM++ 2M SDE Heun": DPMpp2MSDEHeun,
    "DPM++ 2M SDE Heun Karras": DPMpp2MSDEHeun,
    "DPM++ 2M SDE Heun Exponential": DPMpp2MSDEHeun,
    "DPM++ 3M SDE": DPMpp3MSDE,
    "DPM++ 3M SDE Karras": DPMpp3MSDE,
    "LMS": LMS,
    "LMS Karras": LMS,
    "DPM2": DPM2,
    "DPM2 a": DPM2Ancestral,
    "DDPM": EulerAncestral,
    "DPM++ 2S a": DPMpp2SAncestral,
    "DPM++ 2S a Karras": DPMpp2SAncestral,
    "UniPC": UniPC,
    "LCM": LCM,
    "Restart": Restart,
    "DPM fast": DPMFast,
    "DPM adaptive": DPMAdaptive,
    "PLMS": LMS,  # ldm's pseudo-LMS: the multistep family on the discrete schedule
    "DPM2 Karras": DPM2,
    "DPM2 a Karras": DPM2Ancestral,
}


def sampler_names() -> List[str]:
    return sorted(SAMPLERS.keys())


def build_sampler(name: str, schedule: Schedule, strict: bool = False) -> Sampler:
    """``strict=False`` falls back to Euler a on an unknown name, matching
    the reference's sampler-not-found retry (ref worker.py:456-467)."""
    cls = SAMPLERS.get(name)
    if cls is None:
        if strict:
            raise KeyError(f"unknown sampler '{name}'")
        from ..utils import get_logger

        get_logger("samplers").warning(
            "unknown sampler '%s'; falling back to Euler a", name
        )
        cls = EulerAncestral
    return cls(schedule)
