"""Hybrid Monte Carlo over the systems of systems.py (the reference's
nf/hmc.py), for one chain or C independent chains at once.

``HMC(simulation, ...)`` keeps the reference's constructor and its
``generate_v`` / ``run_sim`` / ``hmc`` methods.  ``init_pos`` is one
configuration ([W]; ``LJ``, ``EAM``: [n, dim]) -- one chain, with the reference's
shapes -- or a batch ([C, W]; [C, n, dim]): C chains that share every launch.
One epoch is one ``randn``, one trajectory launch (systems ``integration_step``),
one ``rand`` and one Metropolis launch (nfk_hmc_accept); nothing in the loop
waits for the device and nothing is printed.  On the CPU, in fp64 or with the
simulation's ``use_kernels`` or ``fused_dynamics`` switched off the same steps
run as torch ops.  ``hmc(..., one_launch=True)`` draws the random numbers of
many epochs in bulk and runs all of them in ONE launch (nfk_hmc_run.hip).
``EAM`` takes the same kernels (nfk_eam_trajectory up to 6,144 chains per
launch, the per-step force path above that; nfk_eam_hmc_run), so its
per-epoch Metropolis step is nfk_hmc_accept too, whose ``expf`` may decide an
exact near-tie differently from ``torch.exp``.  At the Fe shape a trajectory is
one wave's serial force loop in either form: the launch saves 1-7 % up to
6,144 rows and nothing on ``hmc(500)``.

As in the reference the default test accepts on the potential alone,
``exp((U_old - U_new) * beta)`` (hmc.py:56), and the default integrator is the
reference's lagged-force scheme.  ``scheme="verlet"`` with ``hamiltonian=True``
is the correct sampler: velocity Verlet and ``+ K_old - K_new`` in the
exponent, K = 0.5 sum v^2.  The integrators are unit-mass, as the reference's
are, so ``hamiltonian=True`` requires ``mass=None``.

Unlike the reference's constructor, a simulation that holds no position yet is
accepted (pass ``init_pos`` here or to ``hmc``).
"""
from __future__ import annotations

import math

import torch
from torch.distributions import MultivariateNormal

from . import kernels as K_
from .systems import EAM, LJ, _SCHEMES

__all__ = ["HMC"]


class HMC:
    def __init__(self, simulation, init_pos=None, path_len=1, dt=None, mass=None, dim=3, beta=1.0,
                 init_beta=None, scheme="reference", hamiltonian=False):
        if hamiltonian and mass is not None:
            raise ValueError("hamiltonian=True needs mass=None: the integrators are unit-mass")
        self.simulation = simulation
        self.dt = dt
        self.path_len = path_len
        self.beta = beta
        self.dim = dim
        self.scheme = scheme
        self.hamiltonian = hamiltonian
        self.mass = mass
        self.init_beta = beta if init_beta is None else init_beta
        self.naccept = None
        self._vd = self._vc = None
        if init_pos is not None:
            self.simulation.set_position(init_pos)
        self.position = simulation.get_position()
        self.potential = None if self.position is None else simulation.get_potential()

    # ------------------------------------------------------------------ velocities
    @property
    def nparticles(self):
        return self.simulation.nparticles

    @property
    def width(self):
        return self.dim * self.nparticles

    def _mass_inverse(self):
        """1/m per coordinate, [W] (hmc.py:24)."""
        mass = torch.ones(self.nparticles) if self.mass is None else torch.as_tensor(self.mass)
        return (1 / mass).expand(self.dim, self.nparticles).transpose(0, 1).flatten()

    @property
    def v_dist(self):
        """The reference's N(0, diag(1/m) / init_beta), on the CPU."""
        if self._vd is None or self._vd[0] != self.width:
            self._vd = (self.width, MultivariateNormal(torch.zeros(self.width),
                                                       torch.diag(self._mass_inverse()) / self.init_beta))
        return self._vd[1]

    def _like(self):
        """(device, dtype, chains, single) of the simulation's held position."""
        x = self.simulation.get_position()
        if x is None:
            raise ValueError("the simulation holds no position: pass init_pos")
        chains = x.numel() // self.width
        if chains * self.width != x.numel():
            raise ValueError("a position of %d elements is no batch of %d coordinates" % (x.numel(), self.width))
        return x.device, x.dtype, chains, x.numel() == self.width and x.dim() <= self._single_dims()

    def _single_dims(self):
        return 2 if isinstance(self.simulation, (LJ, EAM)) else 1  # their positions are [..., n, dim]

    def _var(self, device, dtype):
        """The velocities' variances, [W], kept per device: no copy inside the epoch loop."""
        key = (device, dtype, self.width)
        if self._vc is None or self._vc[0] != key:
            self._vc = (key, (self._mass_inverse() / self.init_beta).to(device=device, dtype=dtype))
        return self._vc[1]

    def log_prob(self, v):
        """v_dist.log_prob in closed form, per row of v: [C]."""
        v = v.reshape(-1, self.width)
        var = self._var(v.device, v.dtype)
        return -0.5 * (self.width * math.log(2 * math.pi) + (v * v / var).sum(1)) - 0.5 * var.log().sum()

    def generate_v(self):
        """One draw per chain of the held position, on its device: (v, log_prob).
        One chain: v [W], log_prob [1], the reference's shapes."""
        v = self._draw()
        return v, self.log_prob(v)

    def _draw(self):
        device, dtype, chains, single = self._like()
        v = torch.randn(chains, self.width, device=device, dtype=dtype) * self._var(device, dtype).sqrt()
        return v.flatten() if single else v

    def run_sim(self, v=None):
        if v is None:
            v, log_prob = self.generate_v()
        else:
            log_prob = self.log_prob(v)
        self.simulation.set_velocity(v)
        position, potential = self.simulation.integration_step(self.path_len, self.dt, scheme=self.scheme)
        return position, potential, log_prob

    # ---------------------------------------------------------------------- chains
    @staticmethod
    def _kinetic(v, chains):
        v = v.reshape(chains, -1)
        return 0.5 * (v * v).sum(1)

    def _accept(self, x_cur, x_new, u_cur, u_new, k_cur, k_new, r, naccept):
        """hmc.py:56-63 over the chains, in place in x_cur, u_cur and naccept."""
        sim = self.simulation
        if (getattr(sim, "use_kernels", True) and getattr(sim, "fused_dynamics", True) and x_cur.is_cuda
                and x_cur.dtype == torch.float32 and u_cur.dtype == torch.float32):
            K_.hmc_accept(x_cur, x_new, u_cur, u_new.contiguous(), r, naccept, beta=self.beta, k_cur=k_cur,
                          k_new=k_new)
            return
        d = u_cur - u_new
        if k_cur is not None:
            d = (d + k_cur) - k_new
        acc = r < torch.exp(d * self.beta)  # a NaN exponent compares false: rejected
        x_cur.copy_(torch.where(acc.unsqueeze(1), x_new, x_cur))
        u_cur.copy_(torch.where(acc, u_new, u_cur))
        naccept += acc.to(torch.int32)

    def hmc(self, epochs=1, init_pos=None, record=True, one_launch=False, draw_bytes=1 << 28):
        """``epochs`` moves of every chain.  Returns the reference's 4-tuple:
        positions [epochs, C, W] and potentials [epochs, C] (entry i is the
        state BEFORE move i, hmc.py:53-54; one chain: [epochs, W] and
        [epochs]), the last velocity log_prob and the acceptance rate, a float
        (the mean over chains; the call's one host synchronisation).
        ``record=False`` stores nothing per epoch and returns the final
        positions and potentials in the first two slots.  ``self.naccept``
        holds the per-chain counts.

        ``one_launch=True`` draws the random numbers of many epochs at once
        and runs those epochs in ONE launch (nfk_hmc_run.hip) instead of a
        trajectory and a Metropolis launch per epoch.  The run is cut into
        segments of ``e = max(1, min(remaining, draw_bytes // (4 * C * (W + 1))))``
        epochs; a segment draws, in this order,

            v = torch.randn(e, C, W, device=..., dtype=...) * sd    # sd = self._var(...).sqrt()
            r = torch.rand(e, C, device=..., dtype=...)

        and epoch i of the segment uses ``v[i]`` and ``r[i]``.  The result
        depends on the seed and on ``draw_bytes`` alone, never on the route:
        where the simulation does not take the kernel (CPU, fp64, a shape
        beyond its limits, ``use_kernels`` or ``fused_dynamics`` off) the
        segment runs as the per-epoch steps fed the same draws, and without
        ``hamiltonian`` the two routes agree bit for bit (with it, the kernel
        sums the kinetic energies in its own order, include/nfk.h).  The draw
        order differs from the default path's (v, r, v, r, ...) unless a
        segment is one epoch long.  ``one_launch=False`` is the per-epoch path,
        unchanged."""
        if one_launch:
            return self._hmc_segments(epochs, init_pos, record, draw_bytes)
        sim = self.simulation
        if init_pos is not None:
            sim.set_position(init_pos)
        device, dtype, chains, single = self._like()
        shape = sim.get_position().shape
        with torch.no_grad():
            x_cur = sim.get_position().detach().reshape(chains, self.width).clone()
            u_cur = sim.get_potential().detach().reshape(chains).clone()
        naccept = torch.zeros(chains, dtype=torch.int32, device=device)
        if record:
            positions = torch.empty(epochs, chains, self.width, dtype=dtype, device=device)
            potentials = torch.empty(epochs, chains, dtype=u_cur.dtype, device=device)
        v = None
        for i in range(epochs):
            if record:
                positions[i].copy_(x_cur)
                potentials[i].copy_(u_cur)
            sim.set_position(x_cur.view(shape))
            v = self._draw()
            sim.set_velocity(v)
            x_new, u_new = sim.integration_step(self.path_len, self.dt, scheme=self.scheme)
            k_cur = k_new = None
            if self.hamiltonian:
                k_cur, k_new = self._kinetic(v, chains), self._kinetic(sim.get_velocity(), chains)
            r = torch.rand(chains, device=device, dtype=u_cur.dtype)
            x_new = x_new.reshape(chains, self.width)
            self._accept(x_cur, x_new if x_new.stride(-1) == 1 else x_new.contiguous(), u_cur,
                         u_new.reshape(chains), k_cur, k_new, r, naccept)
        sim.set_position(x_cur.view(shape))
        log_prob = None if v is None else self.log_prob(v)  # the reference returns the last draw's
        self.naccept = naccept
        self.position = x_cur.flatten() if single else x_cur
        self.potential = u_cur
        rate = float(naccept.double().mean()) / epochs if epochs else 0.0
        if not record:
            return self.position, (u_cur[0] if single else u_cur), log_prob, rate
        if single:
            return positions[:, 0], potentials[:, 0], log_prob, rate
        return positions, potentials, log_prob, rate

    def _hmc_segments(self, epochs, init_pos, record, draw_bytes):
        """``hmc(one_launch=True)``: bulk draws and one launch per segment."""
        sim = self.simulation
        if self.scheme not in _SCHEMES:
            raise ValueError("scheme must be 'reference' or 'verlet', got %r" % (self.scheme,))
        if init_pos is not None:
            sim.set_position(init_pos)
        device, dtype, chains, single = self._like()
        shape = sim.get_position().shape
        W = self.width
        with torch.no_grad():
            x_cur = sim.get_position().detach().reshape(chains, W).clone()
            u_cur = sim.get_potential().detach().reshape(chains).clone()
        naccept = torch.zeros(chains, dtype=torch.int32, device=device)
        positions = potentials = None
        if record:
            positions = torch.empty(epochs, chains, W, dtype=dtype, device=device)
            potentials = torch.empty(epochs, chains, dtype=u_cur.dtype, device=device)
        sd = self._var(device, dtype).sqrt()
        run = getattr(sim, "_hmc_run", None)
        v = v_last = None
        done = 0
        while done < epochs:
            e = max(1, min(epochs - done, int(draw_bytes) // (4 * max(1, chains) * (W + 1))))
            v = torch.randn(e, chains, W, device=device, dtype=dtype) * sd
            r = torch.rand(e, chains, device=device, dtype=u_cur.dtype)
            pos = positions[done:done + e] if record else None
            pot = potentials[done:done + e] if record else None
            v_out = None if run is None else torch.empty_like(x_cur)
            if run is not None and run(x_cur, u_cur, naccept, v, r, shape=shape, path_len=self.path_len,
                                       dt=self.dt, sch=_SCHEMES[self.scheme], beta=self.beta,
                                       hamiltonian=self.hamiltonian, v_last=v_out, pos_rec=pos, pot_rec=pot):
                v_last = v_out.view(shape)
            else:
                for i in range(e):
                    if record:
                        pos[i].copy_(x_cur)
                        pot[i].copy_(u_cur)
                    sim.set_position(x_cur.view(shape))
                    sim.set_velocity(v[i].flatten() if single else v[i])
                    x_new, u_new = sim.integration_step(self.path_len, self.dt, scheme=self.scheme)
                    k_cur = k_new = None
                    if self.hamiltonian:
                        k_cur, k_new = self._kinetic(v[i], chains), self._kinetic(sim.get_velocity(), chains)
                    x_new = x_new.reshape(chains, W)
                    self._accept(x_cur, x_new if x_new.stride(-1) == 1 else x_new.contiguous(), u_cur,
                                 u_new.reshape(chains), k_cur, k_new, r[i], naccept)
                v_last = sim.get_velocity()
            done += e
        sim.set_position(x_cur.view(shape))
        if v_last is not None:
            sim.set_velocity(v_last)
        log_prob = None if v is None else self.log_prob(v[-1])  # the reference returns the last draw's
        self.naccept = naccept
        self.position = x_cur.flatten() if single else x_cur
        self.potential = u_cur
        rate = float(naccept.double().mean()) / epochs if epochs else 0.0
        if not record:
            return self.position, (u_cur[0] if single else u_cur), log_prob, rate
        if single:
            return positions[:, 0], potentials[:, 0], log_prob, rate
        return positions, potentials, log_prob, rate
