"""Priors and targets of the reference's applications layer
(applications/src/systems.py): EinsteinCrystal, GaussianMixture and LJ, with
the reference's constructor signatures and method names.

fp32 tensors on the HIP device take the kernels of nfk_systems.hip (one launch
per log_prob / potential, one per backward; no [B, N, N] temporary for LJ)
and, for ``integration_step``, of nfk_dynamics.hip (a whole batch of
trajectories in one launch); ``langevin`` is the thermostatted counterpart
(nfk_langevin.hip, the noise generated in the kernel: rng.py).
Every other input -- CPU tensors, other float dtypes, parameters that require
grad, shapes the kernels do not take -- runs the plain-torch restatement in
this module: the same formulas in the input's dtype, differentiable by
autograd.  (Unlike the flow layers, which refuse CPU tensors, these classes
are plain formulas and serve as their own CPU companions.)

As priors of ``NormalizingFlowModel`` the Einstein crystal and the mixture get
what the Normal prior gets: the kernel with ``+ sign * log|det|`` fused, a
status word for the reference's NaN ``ValueError``, an autograd node under
training and HIP-graph capture (models._prior_log_prob).

``EAM`` is the Fe target without LAMMPS: the embedded-atom energy of a setfl
table file (``read_setfl``) over every periodic image within the cutoff, by
the kernels of nfk_eam.hip.

``Switch`` integrates Langevin dynamics on the lambda-mixed Hamiltonian
between a normalised reference (the Einstein crystal) and a target and
accumulates the switching work (nfk_switch.hip): the free energy without a
flow, app.fe_switching.

Out of scope: LAMMPS itself and plotting.  HMC is in hmc.py, the BAR estimator
in bar.py, MBAR in mbar.py.
"""
from __future__ import annotations

import math

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import kernels as K_
from .flows import check_status

__all__ = ["EinsteinCrystal", "GaussianMixture", "LJ", "EAM", "Switch", "read_xyz", "load_position", "read_setfl"]

_LOG_2PI = math.log(2 * math.pi)


# ---------------------------------------------------------------------------
# files
def read_xyz(path):
    """Frames of an XYZ file in the format utils.write_coord emits (a count
    line, a comment line, then ``type x y z`` lines) as a float32 tensor
    [nframes, natoms, 3]."""
    with open(path) as f:
        lines = f.read().splitlines()
    frames, i = [], 0
    while i < len(lines):
        if not lines[i].strip():
            i += 1
            continue
        n = int(lines[i].split()[0])
        rows = lines[i + 2:i + 2 + n]
        if len(rows) != n:
            raise ValueError("%s: frame %d is truncated (%d of %d atoms)" % (path, len(frames), len(rows), n))
        frames.append([[float(v) for v in r.split()[1:4]] for r in rows])
        i += n + 2
    if not frames:
        raise ValueError("%s: no frames" % path)
    if any(len(fr) != len(frames[0]) for fr in frames):
        raise ValueError("%s: frames with different atom counts" % path)
    return torch.tensor(np.asarray(frames, dtype=np.float32))


def load_position(path):
    """utils.load_position: the frames of an XYZ file, [nframes, natoms * 3]."""
    return read_xyz(path).flatten(start_dim=1)


def read_setfl(path):
    """A single-element setfl table file (LAMMPS ``eam/alloy``; ``eam/fs`` has
    the same layout for one element): 3 comment lines, ``Nelements name``,
    ``Nrho drho Nr dr rc``, the element line, then Nrho values of F(rho), Nr of
    f(r) and Nr of z(r) = r phi(r), free-format across lines.  Returns a dict
    with ``nrho, drho, nr, dr, rc``, the fp64 arrays ``F, f, z``, ``element``
    (its name) and ``element_line`` (the four tokens of the element line).
    More than one element raises ``NotImplementedError``."""
    with open(path) as fh:
        lines = fh.read().splitlines()
    if len(lines) < 6:
        raise ValueError("%s: not a setfl file (%d lines)" % (path, len(lines)))
    head = lines[3].split()
    if int(head[0]) != 1:
        raise NotImplementedError("%s: %s elements; only single-element setfl files are read" % (path, head[0]))
    grid = lines[4].split()
    nrho, drho, nr, dr, rc = int(grid[0]), _fnum(grid[1]), int(grid[2]), _fnum(grid[3]), _fnum(grid[4])
    vals = np.array([_fnum(t) for ln in lines[6:] for t in ln.split()], dtype=np.float64)
    if len(vals) < nrho + 2 * nr:
        raise ValueError("%s: %d table values, expected %d" % (path, len(vals), nrho + 2 * nr))
    return dict(element=head[1] if len(head) > 1 else "", element_line=lines[5].split(), nrho=nrho, drho=drho,
                nr=nr, dr=dr, rc=rc, F=vals[:nrho].copy(), f=vals[nrho:nrho + nr].copy(),
                z=vals[nrho + nr:nrho + 2 * nr].copy())


def _fnum(tok):
    return float(tok.replace("D", "E").replace("d", "e"))


def _cubic_table(y):
    """The C1 piecewise cubic through the nodes y (fp64, n >= 5): per interval
    m the quadruple (c3, c4, s_m, y_m) of ((c3 p + c4) p + s_m) p + y_m on
    p in [0, 1], with five-point node slopes inside and one- and two-sided
    differences at the ends.  Returns ([n - 1, 4], the n node slopes)."""
    y = np.asarray(y, dtype=np.float64)
    n = len(y)
    if n < 5:
        raise ValueError("a table needs at least 5 points, got %d" % n)
    s = np.empty(n)
    s[0] = y[1] - y[0]
    s[1] = (y[2] - y[0]) / 2
    s[2:n - 2] = ((y[:n - 4] - y[4:]) + 8 * (y[3:n - 1] - y[1:n - 3])) / 12
    s[n - 2] = (y[n - 1] - y[n - 3]) / 2
    s[n - 1] = y[n - 1] - y[n - 2]
    dy = y[1:] - y[:-1]
    c4 = 3 * dy - 2 * s[:-1] - s[1:]
    c3 = s[:-1] + s[1:] - 2 * dy
    return np.stack((c3, c4, s[:-1], y[:-1]), axis=1), s


def _cubic(q, p):
    return ((q[..., 0] * p + q[..., 1]) * p + q[..., 2]) * p + q[..., 3]


def _load_traj(src):
    if torch.is_tensor(src):
        return src.float()
    if isinstance(src, str):
        if src.endswith(".npy"):
            return torch.from_numpy(np.load(src, allow_pickle=False)).float()
        if src.endswith(".pt"):
            return torch.as_tensor(torch.load(src, map_location="cpu", weights_only=True)).float()
        return read_xyz(src)
    return torch.as_tensor(np.asarray(src)).float()


def _centers(centers, dim, device):
    if isinstance(centers, str):
        return load_position(centers).reshape(-1, dim).to(device)
    if torch.is_tensor(centers):
        return centers.float().to(device)
    return torch.tensor(centers).float().to(device)


def _wrap(v, boxlength):
    """The reference's single wrap: v - (|v| > 0.5 L) sign(v) L."""
    return v - (torch.abs(v) > 0.5 * boxlength) * torch.sign(v) * boxlength


def _rows(x, width):
    """x as [B, width] rows with unit column stride (a view when it already is)."""
    z = x.reshape(-1, width)
    return z if z.shape[1] <= 1 or z.stride(1) == 1 else z.contiguous()


def _raise_nan(x, who):
    if bool((x != x).any()):
        raise ValueError("Expected value argument to be within the support (IndependentConstraint("
                         "Real(), 1)) of the distribution %s, but found invalid values (NaN)"
                         % type(who).__name__)


_SCHEMES = {"reference": 0, "verlet": 1}


class _Dynamics:
    """The state and the integrator of systems.py:297-338 and 382-401, batched:
    ``set_position`` / ``set_velocity`` / ``get_position`` / ``get_velocity`` /
    ``get_potential`` and ``integration_step``.

    A position is one configuration or a batch of independent ones, [W] or
    [B, W] (``LJ``, ``EAM``: [..., n, dim]).  The reference's own batch, one flattened
    vector of B configurations, gives the same numbers; results come back in
    the shape that was given, the potential as [B].

    ``scheme="reference"`` is the reference's integrator, which evaluates the
    "new" force at the old position (G_k = F(x_{k-1})) and is therefore not
    time-reversible; ``scheme="verlet"`` is velocity Verlet (G_k = F(x_k)).
    Per step, in the input's dtype and in this order:

        x' = (x + v*dt) + (G*0.5)*dt**2
        Gn = F(x' if verlet else x)
        v' = v + (dt*(G + Gn))*0.5

    fp32 device tensors at the kernels' shapes take ONE launch for the whole
    trajectory (nfk_dynamics.hip), bit for bit the per-step path in x and v.
    Everything else -- CPU, fp64, other shapes, ``use_kernels = False`` or
    ``fused_dynamics = False`` -- runs the per-step path: ``get_force`` /
    ``force`` per step plus torch elementwise ops.

    Two deliberate differences from the reference.  Its ``self.force = ...``
    replaces ``GaussianMixture.force``, the method, by a tensor; here the last
    force is ``self.last_force`` and ``force`` stays callable.  And its outputs
    carry an autograd graph that grows by one force evaluation per step; here
    both paths return detached tensors (``get_force`` keeps the
    ``create_graph=True`` spelling)."""

    fused_dynamics = True
    position = None
    velocity = None
    _last_force = None
    _replay = None

    def set_position(self, position):
        self.position = position

    def get_position(self):
        return self.position

    def set_velocity(self, velocity):
        self.velocity = velocity

    def get_velocity(self):
        return self.velocity

    def get_potential(self, x=None):
        return self.potential(self.position if x is None else x)

    @property
    def last_force(self):
        """G after the last ``integration_step``.  The fused launch keeps the
        force in registers, so after one it is evaluated on the first read
        (for the reference scheme at x_{k-1}, reached by one more launch from
        the tensors the step started from)."""
        if self._last_force is None and self._replay is not None:
            x, v, path_len, dt, sch = self._replay
            if sch == 0 and path_len > 0:
                x = self._integrate(x, v, path_len - 1, dt, sch)[0]
            elif path_len > 0:
                x = self.position
            self._last_force = self._force_detached(x)
        return self._last_force

    def _force_detached(self, x):
        with torch.enable_grad():
            return self.get_force(x.detach()).detach()

    def _dyn_fused_ok(self, x, v):
        return (self.fused_dynamics and torch.is_tensor(v) and v.dtype == x.dtype and v.device == x.device
                and self._kernel_ok(x))

    def _integrate(self, x, v, path_len, dt, sch, keep_force=False):
        """(x, v, potential) after path_len steps; x, v in one shape."""
        if self._dyn_fused_ok(x, v):
            xr, vr = self._dyn_rows(x), self._dyn_rows(v)
            xo, vo = torch.empty_like(xr, memory_format=torch.contiguous_format), torch.empty_like(
                vr, memory_format=torch.contiguous_format)
            pot = torch.empty(xr.shape[0], dtype=torch.float32, device=xr.device)
            self._trajectory(xr.detach(), vr.detach(), xo, vo, pot, path_len, dt, sch)
            if keep_force:
                self._last_force, self._replay = None, (x, v, path_len, dt, sch)
            return xo.reshape(x.shape), vo.reshape(x.shape), self._dyn_pot_shape(pot, x)
        x, v = x.detach(), v.detach()
        G = self._force_detached(x)
        for _ in range(path_len):
            xn = (x + v * dt) + (G * 0.5) * dt ** 2
            Gn = self._force_detached(xn if sch else x)
            v = v + (dt * (G + Gn)) * 0.5
            x, G = xn, Gn
        if keep_force:
            self._last_force, self._replay = G, None
        with torch.no_grad():
            return x, v, self.potential(x)

    def _hmc_run(self, x_cur, u_cur, naccept, v, r, *, shape, path_len, dt, sch, beta, hamiltonian,
                 v_last=None, pos_rec=None, pot_rec=None):
        """All ``v.shape[0]`` HMC epochs of the chains x_cur [C, W] in ONE launch
        (nfk_hmc_run.hip), in place in x_cur, u_cur and naccept; ``v`` [E, C, W]
        and ``r`` [E, C] are the draws and ``shape`` is the shape the simulation
        holds the chains' positions in.  Returns False, having done nothing,
        when the tensors or the shape do not take the kernel (CPU, fp64,
        ``use_kernels`` or ``fused_dynamics`` off, shape not supported): the
        caller then runs the per-epoch steps."""
        f32 = torch.float32
        if not (self.fused_dynamics and x_cur.is_cuda and all(
                torch.is_tensor(t) and t.dtype == f32 and t.device == x_cur.device for t in (x_cur, u_cur, v, r))
                and self._hmc_ok(x_cur, shape)):
            return False
        self._hmc_launch(shape, x_cur, u_cur, naccept, v, r, path_len=int(path_len),
                         dt=0.005 if dt is None else dt, scheme=sch, beta=beta, hamiltonian=hamiltonian,
                         v_last=v_last, pos_rec=pos_rec, pot_rec=pot_rec)
        return True

    def integration_step(self, path_len=1, dt=0.005, init_pos=None, init_velocity=None, scheme="reference"):
        """``path_len`` steps of ``dt`` (None: 0.005) from the held position and
        velocity (or ``init_pos`` / ``init_velocity``); returns (position,
        potential) as the reference does and holds the final state in
        ``self.position`` / ``self.velocity``."""
        if scheme not in _SCHEMES:
            raise ValueError("scheme must be 'reference' or 'verlet', got %r" % (scheme,))
        if init_pos is not None:
            self.set_position(init_pos)
        if init_velocity is not None:
            self.set_velocity(init_velocity)
        if dt is None:
            dt = 0.005
        path_len = int(path_len)
        if path_len < 0:
            raise ValueError("path_len must be >= 0")
        x = self.position
        x, v, pot = self._integrate(x, self.velocity.reshape(x.shape), path_len, dt, _SCHEMES[scheme],
                                    keep_force=True)
        self.position, self.velocity = x, v
        return x, pot

    # ------------------------------------------------------------------ Langevin (NVT)
    _zero_momentum_default = False

    def _lv_nd(self, x):
        """(particles, dim) of a row of x."""
        return self.nparticles, self.dim

    def _lv_ok(self, x, nd):
        return True

    def _closing_potential(self, x):
        """The potential of a Langevin state or frame, [B]."""
        with torch.no_grad():
            return self.potential(x).reshape(-1)

    def langevin(self, nsteps, dt=0.005, gamma=10.0, kT=1.0, mass=1.0, seed=0, init_pos=None,
                 init_velocity=None, record_every=0, zero_momentum=None, step0=0, row_base=0):
        """``nsteps`` steps of Langevin dynamics at temperature ``kT`` (the
        reference's ``fix langevin T T 0.1 seed zero yes``: ``gamma`` = 10 is its
        damping time 0.1) from the held position and velocity (or ``init_pos``
        / ``init_velocity``), by the BAOAB splitting.  Per step, in the
        input's dtype and in this order:

            v = v + hb*F;  x = x + hd*v;  v = c1*v + c2*xi;  x = x + hd*v
            F = force(x);  v = v + hb*F

        with hb = 0.5 dt / mass, hd = 0.5 dt, c1 = exp(-gamma dt), c2 =
        sqrt(kT / mass (1 - c1^2)) (evaluated in double; rounded to fp32 once
        for fp32 inputs) and xi the normals of ``rng.philox_normal`` at
        (``seed``, absolute step ``step0 + k``, particle, row ``row_base + b``).
        ``zero_momentum`` (default: True for LJ and EAM, False for
        EinsteinCrystal and GaussianMixture) removes the noise's mean over a
        row's particles, so the total momentum stays where it is; a missing
        velocity (``get_velocity() is None``) is drawn as sqrt(kT / mass) times
        the tag-1 normals of step ``step0``, mean removed likewise.  Positions
        are not wrapped.

        Returns (position, potential) and holds the final state as
        ``integration_step`` does; with ``record_every > 0`` also the frames
        after every step whose absolute index is a multiple of it
        ([(step0 + nsteps) // record_every - step0 // record_every, B, ...]:
        ``nsteps // record_every`` from step 0) and their potentials.

        fp32 device tensors at the kernels' shapes run whole chunks of at most
        ``config.LANGEVIN_STEPS_PER_LAUNCH`` steps per launch (nfk_langevin.hip;
        no host sync inside a run).  The noise is keyed by the absolute step
        and F is recomputed from x, so a run equals, bit for bit, the same run
        cut into chunks, continued with ``step0``, or split over row blocks
        with ``row_base``.  CPU, fp64, other shapes, ``use_kernels = False``
        and ``fused_dynamics = False`` run the per-step path, on the device
        with the bits of the launch."""
        from . import config, rng
        if init_pos is not None:
            self.set_position(init_pos)
        if init_velocity is not None:
            self.set_velocity(init_velocity)
        nsteps, record_every, step0, row_base, seed = (int(nsteps), int(record_every), int(step0), int(row_base),
                                                       int(seed))
        if nsteps < 0 or record_every < 0 or step0 < 0:
            raise ValueError("nsteps, record_every and step0 must be >= 0")
        if not (dt > 0 and gamma >= 0 and kT >= 0 and mass > 0):
            raise ValueError("langevin needs dt > 0, gamma >= 0, kT >= 0 and mass > 0")
        zm = self._zero_momentum_default if zero_momentum is None else bool(zero_momentum)
        x = self.position
        n, dim = nd = self._lv_nd(x)
        rows = x.numel() // (n * dim)
        c1 = math.exp(-gamma * dt)
        consts = (0.5 * dt / mass, 0.5 * dt, c1, math.sqrt(kT / mass * (1.0 - c1 * c1)))
        vscale = math.sqrt(kT / mass)
        if x.dtype == torch.float32:
            consts = tuple(float(np.float32(c)) for c in consts)
            vscale = float(np.float32(vscale))
        if self.velocity is None:
            self.velocity = vscale * rng.philox_normal(seed, rows, n, dim, step0, row_base, tag=1, zero_mean=zm,
                                                       device=x.device, dtype=x.dtype).reshape(x.shape)
        v = self.velocity.reshape(x.shape)
        nframes = (step0 + nsteps) // record_every - step0 // record_every if record_every else 0
        # (EAM's row cap on integration_step does not apply: the launch won at every measured size)
        if _Dynamics._dyn_fused_ok(self, x, v) and self._lv_ok(x, nd):
            xr, vr = self._dyn_rows(x).detach(), self._dyn_rows(v).detach()
            xo = torch.empty_like(xr, memory_format=torch.contiguous_format)
            vo = torch.empty_like(vr, memory_format=torch.contiguous_format)
            pot = torch.empty(rows, dtype=torch.float32, device=xr.device)
            frames = pots = None
            if record_every:
                frames = torch.empty(nframes, rows, n * dim, dtype=torch.float32, device=xr.device)
                pots = torch.empty(nframes, rows, dtype=torch.float32, device=xr.device)
            cap = max(1, int(config.LANGEVIN_STEPS_PER_LAUNCH))
            done = f0 = 0
            while True:
                m, s0 = min(cap, nsteps - done), step0 + done
                fm = (s0 + m) // record_every - s0 // record_every if record_every else 0
                self._langevin_launch(xr, vr, xo, vo, pot, nd, nsteps=m, consts=consts, seed=seed, step0=s0,
                                      row_base=row_base, zero_mean=zm, record_every=record_every,
                                      pos_rec=None if frames is None else frames[f0:f0 + fm],
                                      pot_rec=None if pots is None else pots[f0:f0 + fm])
                done, f0, xr, vr = done + m, f0 + fm, xo, vo
                if done >= nsteps:
                    break
            x, v = xo.reshape(x.shape), vo.reshape(x.shape)
            if frames is not None:
                frames = frames.reshape(nframes, *x.shape)
        else:
            x, v = x.detach(), v.detach()
            hb, hd, c1, c2 = consts
            F = self._force_detached(x)
            frames, pots = [], []
            for k in range(nsteps):
                xi = rng.philox_normal(seed, rows, n, dim, step0 + k, row_base, tag=0, zero_mean=zm,
                                       device=x.device, dtype=x.dtype).reshape(x.shape)
                v = v + hb * F
                x = x + hd * v
                v = c1 * v + c2 * xi
                x = x + hd * v
                F = self._force_detached(x)
                v = v + hb * F
                if record_every and (step0 + k + 1) % record_every == 0:
                    frames.append(x)
                    pots.append(self._closing_potential(x))
            pot = self._closing_potential(x)
            if record_every:
                frames = torch.stack(frames) if frames else x.new_empty((0,) + tuple(x.shape))
                pots = torch.stack(pots) if pots else pot.new_empty((0, rows))
        self.position, self.velocity = x, v
        self._last_force, self._replay = None, (x, v, 1, dt, 1)  # last_force: F(position), on the first read
        pot = self._dyn_pot_shape(pot, x)
        if record_every:
            return x, pot, frames, pots
        return x, pot


class _SimData:
    """The trajectory holder of the reference's SimData (systems.py:107-142):
    ``traj`` [frames, ...] on ``self.device``, ``sample`` and ``update_data``."""

    def sample(self, nsamples, flatten=True, random=True):
        if random:
            idx = torch.randint(len(self.traj), [nsamples]).to(self.traj.device)
            samples = self.traj.index_select(0, idx)
        else:
            samples = self.traj[:nsamples]
        return samples.reshape(nsamples, -1) if flatten else samples

    def update_data(self, file, append=False):
        """Replace the held trajectory by ``file``'s frames (a tensor, ``.npy``,
        ``.pt`` or XYZ), or append them."""
        traj = _load_traj(file).to(self.device)
        self.traj = torch.cat((self.traj, traj.reshape(len(traj), *self.traj.shape[1:])), 0) if append else traj


class _KernelBacked(_Dynamics):
    """Shared dispatch: ``use_kernels = False`` on an object forces its torch path."""

    use_kernels = True
    _validate_args = True  # the components are MultivariateNormals with torch's default validation

    def _on_device(self, x, *params):
        return (self.use_kernels and torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32
                and all(p.device == x.device and p.dtype == torch.float32 and not p.requires_grad
                        for p in params))

    def _fused(self, z, logdet, sign, status):
        """log_prob(z) + sign * logdet by the kernel; z: [B, width] fp32 on the device."""
        z = _rows(z, self.width)
        if torch.is_grad_enabled() and z.requires_grad:
            lp = self._fn.apply(z, self, status)
            return lp if logdet is None else (lp + logdet if sign >= 0 else lp - logdet)
        out = torch.empty(z.shape[0], dtype=torch.float32, device=z.device)
        self._launch(z.detach(), out, logdet, sign, status)
        return out

    def log_prob(self, x):
        if self._kernel_ok(x):
            status = torch.zeros(1, dtype=torch.int32, device=x.device)
            out = self._fused(x, None, 1, status)
            check_status(status, 0, prior=self)  # a NaN row: torch's ValueError (config.STRICT_CHECKS)
            return out
        return self._log_prob_torch(x)

    def potential(self, x):
        return -self.log_prob(x)

    def get_force(self, x):
        x.requires_grad_()
        pot = self.potential(x)
        return -torch.autograd.grad(pot, x, torch.ones_like(pot), create_graph=True)[0]

    def _dyn_rows(self, t):
        return _rows(t, self.width)

    def _dyn_pot_shape(self, pot, x):
        return pot


# ---------------------------------------------------------------------------
class _EinsteinFn(torch.autograd.Function):
    """nfk_einstein_logprob, differentiable in z: gz = -alpha dev_wrapped g."""

    @staticmethod
    def forward(ctx, z, prior, status):
        out = torch.empty(z.shape[0], dtype=torch.float32, device=z.device)
        prior._launch(z, out, None, 1, status)
        ctx.save_for_backward(z)
        ctx.prior = prior
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        z, = ctx.saved_tensors
        p = ctx.prior
        gz = torch.empty(z.shape, dtype=torch.float32, device=z.device)
        K_.einstein_logprob_bwd(z, p.centers, g.contiguous(), gz, scale=p._consts()[0], boxlength=p.boxlength)
        return gz, None, None


class EinsteinCrystal(_KernelBacked):
    """systems.py:340-375: independent N(centre_i, I/alpha) per atom, with one
    minimum-image wrap of the deviation when ``boxlength`` is not None (0 is
    legal and wraps nothing)."""

    _fn = _EinsteinFn

    def __init__(self, centers, dim=3, boxlength=None, alpha=50, device="cpu"):
        self.device = device
        self.centers = _centers(centers, dim, device)
        self.natoms = self.centers.shape[0]
        self.alpha = alpha
        self.dim = dim
        self.boxlength = boxlength
        self._ck = None

    @property
    def width(self):
        return self.natoms * self.dim

    def _norm_consts(self, dtype):
        """(scale_tril diagonal, half_log_det) of MultivariateNormal(0, I/alpha)
        as torch evaluates them in ``dtype`` (CPU scalars: no device sync)."""
        scale = (1 / self.alpha * torch.ones((), dtype=dtype)).sqrt()
        return scale, scale.log().expand(self.dim).sum()

    def _consts(self):
        key = (self.alpha, self.dim)
        if self._ck is None or self._ck[0] != key:
            s, h = self._norm_consts(torch.float32)
            self._ck = (key, (float(s), float(h)))
        return self._ck[1]

    def _cache_key(self):
        c = self.centers
        return (c.data_ptr(), c._version, self.alpha, self.dim, self.boxlength)

    def _kernel_ok(self, x):
        return (self._on_device(x, self.centers) and self.centers.shape == (self.natoms, self.dim)
                and self.centers.is_contiguous() and x.numel() % self.width == 0)

    def _launch(self, z, out, logdet, sign, status):
        scale, hld = self._consts()
        K_.einstein_logprob(z, self.centers, out, scale=scale, hld=hld, boxlength=self.boxlength,
                            logdet=logdet, sign=sign, status=status)

    @property
    def nparticles(self):
        return self.natoms

    def _trajectory(self, x, v, xo, vo, pot, path_len, dt, sch):
        scale, hld = self._consts()
        K_.einstein_trajectory(x, v, xo, vo, pot, self.centers, path_len=path_len, dt=dt, scheme=sch,
                               scale=scale, hld=hld, boxlength=self.boxlength)

    def _lv_ok(self, x, nd):
        return self.dim <= 4  # a lane takes one of the four normals of its atom's call

    def _langevin_launch(self, x, v, xo, vo, pot, nd, **kw):
        scale, hld = self._consts()
        K_.einstein_langevin(x, v, xo, vo, pot, self.centers, scale=scale, hld=hld, boxlength=self.boxlength, **kw)

    def _closing_potential(self, x):
        # on the device the trajectory kernels' closing potential (a launch of zero
        # steps), whose row sum runs in their order: nfk_einstein_logprob's float4
        # form sums in another, and a per-step run is to have the launch's bits
        if self._kernel_ok(x):
            xr = self._dyn_rows(x).detach()
            xo, pot = torch.empty_like(xr, memory_format=torch.contiguous_format), torch.empty(
                xr.shape[0], dtype=torch.float32, device=xr.device)
            self._trajectory(xr, xr, xo, torch.empty_like(xo), pot, 0, 0.0, 1)
            return pot
        return super()._closing_potential(x)

    def _hmc_ok(self, x_cur, shape):
        return self._kernel_ok(x_cur) and K_.einstein_hmc_supported(self.natoms, self.dim)

    def _hmc_launch(self, shape, *args, **kw):
        scale, hld = self._consts()
        K_.einstein_hmc_run(*args, self.centers, scale=scale, hld=hld, boxlength=self.boxlength, **kw)

    def _log_prob_torch(self, x):
        if self._validate_args:
            _raise_nan(x, self)
        c = self.centers if self.centers.dtype == x.dtype else self.centers.to(x.dtype)
        dev = x.reshape(-1, self.natoms, self.dim) - c
        if self.boxlength is not None:
            dev = _wrap(dev, self.boxlength)
        scale, hld = self._norm_consts(x.dtype)
        y = dev / scale.to(x.device)
        lp = -0.5 * (self.dim * _LOG_2PI + (y * y).sum(-1)) - hld.to(x.device)
        return torch.sum(lp, dim=1)

    def sample(self, nsamples, flatten=True):
        with torch.no_grad():
            if isinstance(nsamples, tuple):
                nsamples = nsamples[0]
            c = self.centers
            noise = torch.randn(nsamples, self.natoms, self.dim, dtype=c.dtype, device=c.device)
            samples = c + noise * float(self._norm_consts(torch.float32)[0])
            if self.boxlength is not None:
                samples = _wrap(samples, self.boxlength)
            return samples.reshape(nsamples, -1) if flatten else samples


# ---------------------------------------------------------------------------
class _GmixFn(torch.autograd.Function):
    """nfk_gmix_logprob, differentiable in x: sum_i w_i (-(x - c_i)/var_i) g."""

    @staticmethod
    def forward(ctx, x, prior, status):
        out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        prior._launch(x, out, None, 1, status)
        ctx.save_for_backward(x)
        ctx.prior = prior
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, = ctx.saved_tensors
        p = ctx.prior
        scales, hlds = p._consts()
        gx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        K_.gmix_logprob_bwd(x, p.centers, scales, hlds, g.contiguous(), gx, npart=p.nparticles)
        return gx, None, None


class GaussianMixture(_KernelBacked):
    """systems.py:257-311: ``nparticles`` independent particles, each drawn from
    an equal-weight mixture of N(centre_i, var_i I).  log_prob keeps the
    reference's arithmetic, sum_i (1/M) exp(log N_i(x)) in centre order and
    then log: not a log-sum-exp, so a particle far from every centre gives
    -inf.  ``sample`` draws the components with torch.randint on the device."""

    _fn = _GmixFn

    def __init__(self, centers, vars, npoints=None, dim=3, device="cpu"):
        self.dim = dim
        self.device = device
        self.centers = _centers(centers, dim, device)
        self.ncenters = len(self.centers)
        self.vars = (vars.float() if torch.is_tensor(vars) else torch.tensor(vars).float()).to(device)
        if self.vars.dim() == 0:
            self.vars = self.vars.expand(self.ncenters)
        elif self.vars.numel() == self.ncenters:  # [[v]] per centre (Gaussian_rnvp.yaml): v I all the same
            self.vars = self.vars.reshape(self.ncenters)
        else:
            raise ValueError("vars must be a scalar or one variance per centre, got shape %s"
                             % (tuple(self.vars.shape),))
        self.nparticles = self.ncenters if npoints is None else npoints
        self._ck = None

    @property
    def width(self):
        return self.nparticles * self.dim

    def _norm_consts(self, dtype):
        """Per-centre (scale_tril diagonal, half_log_det) as torch evaluates
        them for MultivariateNormal(c_i, var_i I) in ``dtype``."""
        scales = self.vars.to(dtype).sqrt()
        return scales, scales.log().unsqueeze(1).expand(self.ncenters, self.dim).sum(1)

    def _cache_key(self):
        c, v = self.centers, self.vars
        return (c.data_ptr(), c._version, v.data_ptr(), v._version, self.nparticles, self.dim)

    def _consts(self):
        key = self._cache_key()
        if self._ck is None or self._ck[0] != key:
            with torch.no_grad():
                s, h = self._norm_consts(torch.float32)
                self._ck = (key, (s.contiguous(), h.contiguous()))
        return self._ck[1]

    def _kernel_ok(self, x):
        return (self._on_device(x, self.centers, self.vars) and K_.gmix_supported(self.ncenters, self.dim)
                and self.centers.shape == (self.ncenters, self.dim) and self.centers.is_contiguous()
                and x.numel() % self.width == 0)

    def _launch(self, x, out, logdet, sign, status):
        scales, hlds = self._consts()
        K_.gmix_logprob(x, self.centers, scales, hlds, out, npart=self.nparticles, logdet=logdet,
                        sign=sign, status=status)

    def _log_prob_torch(self, x):
        if self._validate_args:
            _raise_nan(x, self)
        c = self.centers if self.centers.dtype == x.dtype else self.centers.to(x.dtype)
        scales, hlds = self._norm_consts(x.dtype)
        x = x.reshape(-1, self.dim)
        prob = 0
        for i in range(self.ncenters):
            y = (x - c[i]) / scales[i]
            lp = -0.5 * (self.dim * _LOG_2PI + (y * y).sum(-1)) - hlds[i]
            prob = prob + 1 / self.ncenters * torch.exp(lp)
        return torch.sum(torch.log(prob).reshape(-1, self.nparticles), dim=1)

    def force(self, x):
        return self.get_force(x)

    def _trajectory(self, x, v, xo, vo, pot, path_len, dt, sch):
        scales, hlds = self._consts()
        K_.gmix_trajectory(x, v, xo, vo, pot, self.centers, scales, hlds, path_len=path_len, dt=dt,
                           scheme=sch, npart=self.nparticles)

    def _langevin_launch(self, x, v, xo, vo, pot, nd, **kw):
        scales, hlds = self._consts()
        K_.gmix_langevin(x, v, xo, vo, pot, self.centers, scales, hlds, npart=self.nparticles, **kw)

    def _hmc_ok(self, x_cur, shape):
        return self._kernel_ok(x_cur) and K_.gmix_hmc_supported(self.nparticles, self.dim, self.ncenters)

    def _hmc_launch(self, shape, *args, **kw):
        scales, hlds = self._consts()
        K_.gmix_hmc_run(*args, self.centers, scales, hlds, npart=self.nparticles, **kw)

    def sample(self, nsamples, flatten=True):
        with torch.no_grad():
            if isinstance(nsamples, tuple):
                nsamples = nsamples[0]
            c = self.centers
            n = nsamples * self.nparticles
            which = torch.randint(self.ncenters, (n,), device=c.device)
            scales = self._norm_consts(torch.float32)[0]
            noise = torch.randn(n, self.dim, dtype=c.dtype, device=c.device)
            samples = c.index_select(0, which) + noise * scales.index_select(0, which).unsqueeze(1)
            if flatten:
                return samples.reshape(nsamples, -1)
            return samples.reshape(nsamples, self.nparticles, self.dim)


# ---------------------------------------------------------------------------
class _LJFn(torch.autograd.Function):
    """nfk_lj_potential on [B, n*dim] rows, differentiable in x."""

    @staticmethod
    def forward(ctx, x, lj, n, dim):
        out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        K_.lj_potential(x, out, n=n, dim=dim, **lj._kw())
        ctx.save_for_backward(x)
        ctx.lj, ctx.n, ctx.d = lj, n, dim
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, = ctx.saved_tensors
        gx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        K_.lj_potential_bwd(x, g.contiguous(), gx, n=ctx.n, dim=ctx.d, **ctx.lj._kw())
        return gx, None, None, None


class LJ(_SimData, _Dynamics):
    """systems.py:144-189: Lennard-Jones particles in a periodic cubic box,
    plus the trajectory holder of SimData (``sample``).  ``pos_dir`` may be a
    tensor, a ``.npy`` / ``.pt`` path or an XYZ file.

    ``potential`` keeps the reference's arithmetic: one minimum-image wrap per
    component of the pair vector, ``d + (d == 0)``, ``1/d`` zeroed beyond the
    cutoff, the ``- s6^2 + s6`` shift (s6 = (sigma/cutoff)^6), the final
    ``* inv * d`` factor (zero on the diagonal, for coincident pairs and
    beyond the cutoff) and ``sum / 2``.  ``boxlength=None`` raises TypeError
    as the reference's ``0.5 * None`` does.

    ``force`` is -grad potential (the backward kernel on the device, autograd
    elsewhere).  This is the working form: the reference's ``force`` stops at
    a NameError (``force_mag``, systems.py:220)."""

    use_kernels = True
    _CHUNK_ELEMS = 1 << 24  # pair components per chunk of the torch path

    def __init__(self, pos_dir=None, boxlength=None, device="cpu", epsilon=1., sigma=1., cutoff=None,
                 shift=True):
        self.device = device
        if pos_dir is not None:
            self.traj = _load_traj(pos_dir).to(device)
        self.epsilon = epsilon
        self.sigma = sigma
        self.cutoff = cutoff
        self.shift = shift
        self.boxlength = boxlength

    def _kw(self):
        return dict(boxlength=self.boxlength, sigma=self.sigma, epsilon=self.epsilon, cutoff=self.cutoff,
                    shift=self.shift)

    def _kernel_ok(self, pos):
        return (self.use_kernels and torch.is_tensor(pos) and pos.is_cuda and pos.dtype == torch.float32
                and pos.dim() >= 2 and K_.lj_supported(pos.shape[-2], pos.shape[-1]))

    def potential(self, particle_pos):
        half = 0.5 * self.boxlength  # None: the reference's TypeError
        if self._kernel_ok(particle_pos):
            n, dim = particle_pos.shape[-2:]
            x = _rows(particle_pos, n * dim)
            if torch.is_grad_enabled() and x.requires_grad:
                out = _LJFn.apply(x, self, n, dim)
            else:
                out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
                K_.lj_potential(x.detach(), out, n=n, dim=dim, **self._kw())
            return out.reshape(particle_pos.shape[:-2])
        n, dim = particle_pos.shape[-2:]
        rows = max(1, self._CHUNK_ELEMS // max(1, n * n * dim))
        if particle_pos.dim() < 3 or particle_pos.shape[:-2].numel() <= rows:
            return self._potential_torch(particle_pos, half)
        flat = particle_pos.reshape(-1, n, dim)  # row chunks: no [B, N, N, dim] temporary of the whole batch
        out = torch.cat([self._potential_torch(flat[i:i + rows], half) for i in range(0, flat.shape[0], rows)])
        return out.reshape(particle_pos.shape[:-2])

    def _potential_torch(self, particle_pos, half):
        pair_dist = particle_pos.unsqueeze(-2) - particle_pos.unsqueeze(-3)
        pair_dist = pair_dist - (torch.abs(pair_dist) > half) * torch.sign(pair_dist) * self.boxlength
        distances = torch.linalg.norm(pair_dist, axis=-1)
        scaled_distances = distances + (distances == 0)
        distances_inverse = 1 / scaled_distances
        if self.cutoff is not None:
            distances_inverse = distances_inverse - (distances > self.cutoff) * distances_inverse
        pow_6 = torch.pow(self.sigma * distances_inverse, 6)
        if self.cutoff is not None and self.shift:
            pow_6_shift = (self.sigma / self.cutoff) ** 6
            pair_potential = self.epsilon * 4 * (torch.pow(pow_6, 2) - pow_6 - pow_6_shift ** 2 + pow_6_shift)
        else:
            pair_potential = self.epsilon * 4 * (torch.pow(pow_6, 2) - pow_6)
        pair_potential = pair_potential * distances_inverse * distances
        return torch.sum(pair_potential, axis=(-1, -2)) / 2

    def force(self, particle_pos):
        if self._kernel_ok(particle_pos):
            if self.boxlength is None:
                raise TypeError("unsupported operand type(s) for *: 'float' and 'NoneType' (boxlength=None)")
            n, dim = particle_pos.shape[-2:]
            x = _rows(particle_pos.detach(), n * dim)
            gx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
            K_.lj_potential_bwd(x, torch.ones(x.shape[0], dtype=torch.float32, device=x.device), gx, n=n,
                                dim=dim, **self._kw())
            return -gx.reshape(particle_pos.shape)
        with torch.enable_grad():
            x = particle_pos.detach().requires_grad_()
            pot = self.potential(x)
            return -torch.autograd.grad(pot, x, torch.ones_like(pot))[0]

    @property
    def nparticles(self):
        """Read from the held position: LJ stores no particle count."""
        if self.position is None:
            raise AttributeError("LJ.nparticles needs a position: call set_position first")
        return self.position.shape[-2]

    def get_force(self, x):
        return self.force(x)

    def _dyn_rows(self, t):
        return _rows(t, t.shape[-2] * t.shape[-1])

    def _dyn_pot_shape(self, pot, x):
        return pot.reshape(x.shape[:-2])

    def _trajectory(self, x, v, xo, vo, pot, path_len, dt, sch):
        n, dim = self._traj_nd  # the rows are [n*dim]: _integrate notes the split
        K_.lj_trajectory(x, v, xo, vo, pot, path_len=path_len, dt=dt, scheme=sch, n=n, dim=dim, **self._kw())

    _zero_momentum_default = True

    def _lv_nd(self, x):
        if x.dim() < 2:
            raise ValueError("LJ positions are [..., n, dim]; got shape %s" % (tuple(x.shape),))
        return tuple(x.shape[-2:])

    def _lv_ok(self, x, nd):
        return self.boxlength is not None  # no box: the per-step path raises the reference's TypeError

    def _langevin_launch(self, x, v, xo, vo, pot, nd, **kw):
        K_.lj_langevin(x, v, xo, vo, pot, n=nd[0], dim=nd[1], **self._kw(), **kw)

    def _hmc_ok(self, x_cur, shape):
        # no box: the per-epoch steps raise the reference's TypeError
        return (self.use_kernels and self.boxlength is not None and len(shape) >= 2
                and K_.lj_hmc_supported(shape[-2], shape[-1]))

    def _hmc_launch(self, shape, *args, **kw):
        K_.lj_hmc_run(*args, n=shape[-2], dim=shape[-1], **self._kw(), **kw)

    def _integrate(self, x, v, path_len, dt, sch, keep_force=False):
        if x.dim() < 2:
            raise ValueError("LJ positions are [..., n, dim]; got shape %s" % (tuple(x.shape),))
        if self.boxlength is None:
            raise TypeError("unsupported operand type(s) for *: 'float' and 'NoneType' (boxlength=None)")
        self._traj_nd = tuple(x.shape[-2:])
        return super()._integrate(x, v, path_len, dt, sch, keep_force)


# ---------------------------------------------------------------------------
class _EAMFn(torch.autograd.Function):
    """nfk_eam_potential on [B, n*3] rows, differentiable in x."""

    @staticmethod
    def forward(ctx, x, eam, n):
        out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        K_.eam_potential(x, out, n=n, **eam._kw(x.device))
        ctx.save_for_backward(x)
        ctx.eam, ctx.n = eam, n
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, = ctx.saved_tensors
        gx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        K_.eam_potential_bwd(x, g.contiguous(), gx, n=ctx.n, **ctx.eam._kw(x.device))
        return gx, None, None


class EAM(_SimData, _Dynamics):
    """The Fe target of the reference (systems.py:225-253, a host loop that
    hands one frame at a time to LAMMPS) as an embedded-atom model evaluated
    here: N atoms of one species in a periodic orthorhombic box,

        rho_i = sum_(j,s) f(r_ijs)
        U     = sum_i F(rho_i) + 1/2 sum_i sum_(j,s) z(r_ijs) / r_ijs

    with F, f and z = r phi from a setfl table (``table``: a path or the dict
    ``read_setfl`` returns).  s runs over integer image shifts, r_ijs =
    |x_i - x_j + s L|, and a term counts when 0 < r_ijs <= rc: every periodic
    image inside the cutoff, not only the nearest (at the Fe configs' box the
    cutoff exceeds L/2), self images (i == j, s != 0) included.  Each component
    of x_i - x_j is wrapped once into [-L/2, L/2], then the shifts -n_a..n_a
    with n_a = floor(rc / L_a + 0.5) are visited per axis.  Only exact r == 0
    is skipped: the atom itself, and also a coincident atom, which therefore
    contributes nothing (as LJ's ``d + (d == 0)`` does).

    Each table becomes a C1 piecewise cubic in fp64 (``_cubic_table``; fp32
    copies for the kernel): the interval index is clamped to the table, for r
    the fraction p is clamped to 1, and beyond the last rho node F continues
    as a straight line with the end slope.  The force is the exact gradient of
    that interpolated energy.  To the best of our knowledge this is the scheme
    of LAMMPS's ``pair_eam``; that could not be checked, so no bit parity with
    LAMMPS is claimed.

    ``potential(pos)``: [..., n, 3] -> [...].  fp32 device tensors take
    nfk_eam.hip (one launch per batch, one for the gradient); CPU, fp64,
    n > 256 and ``use_kernels = False`` take the plain-torch restatement in
    the input's dtype, differentiable by autograd and chunked over rows.
    ``boxlength`` is a scalar or (Lx, Ly, Lz).  The class also holds a
    trajectory as the reference's SimData does (``sample``, ``update_data``).

    Dynamics (``integration_step``, ``HMC``): fp32 device tensors with
    n <= 256 take ONE launch per batch of trajectories (nfk_eam_trajectory) and
    ``hmc(one_launch=True)`` one launch per run (nfk_eam_hmc_run), with the
    bits of the per-step path in x, v, the potential and ``last_force``: the
    kernels share the force and energy functions of nfk_eam.hip.  CPU, fp64,
    n > 256, ``use_kernels = False`` and ``fused_dynamics = False`` run the
    per-step path on the force kernel, and so do batches of more than 6,144
    rows, where that path measured 1-10 % faster (at the Fe shape a row is one
    wave's serial force loop in either form: the launch saves 1-7 % below the
    cap and nothing on ``hmc(500)``).  The one observable difference from the
    per-step torch ops: with ``fused_dynamics`` on, the per-epoch Metropolis
    step is nfk_hmc_accept, as for the other systems, and its ``expf`` may
    decide an exact near-tie differently from ``torch.exp``.  Timings: DESIGN.md
    section 12.2.  Time is the unit-mass reduced time of every other system
    here.  With a setfl table in LAMMPS metal units (eV,
    Angstrom) one unit of that time is sqrt(m amu A^2 / eV) = 0.0101805
    sqrt(m) ps for atoms of m g/mol, 0.076079 ps for Fe (55.845): a metal-units
    timestep of 0.001 ps is dt = 0.013144 here, velocities are A per reduced
    time, and beta = 1 / (8.617333e-5 eV/K * T)."""

    use_kernels = True
    fused_dynamics = True
    _CHUNK_ELEMS = 1 << 21  # (i, j) pairs per chunk of the torch path
    _FUSED_ROWS_MAX = 6144  # rows of one trajectory launch; above, the per-step path measured faster

    def __init__(self, table, boxlength, nparticles=None, pos_dir=None, device="cpu"):
        self.device = device
        tab = read_setfl(table) if isinstance(table, str) else table
        self.table = tab
        self.nr, self.dr, self.nrho, self.drho, self.rc = (int(tab["nr"]), float(tab["dr"]), int(tab["nrho"]),
                                                           float(tab["drho"]), float(tab["rc"]))
        if not (self.dr > 0 and self.drho > 0 and self.rc > 0):
            raise ValueError("setfl spacings and cutoff must be positive")
        if len(tab["F"]) != self.nrho or len(tab["f"]) != self.nr or len(tab["z"]) != self.nr:
            raise ValueError("table lengths do not match nrho / nr")
        self.boxlength = boxlength
        box = np.broadcast_to(np.asarray(boxlength, dtype=np.float64), (3,))
        self.box = tuple(float(v) for v in box)
        if not all(v > 0 for v in self.box):
            raise ValueError("box lengths must be positive, got %r" % (boxlength,))
        self.nshift = tuple(int(math.floor(self.rc / v + 0.5)) for v in self.box)
        qf, _ = _cubic_table(tab["f"])
        qz, _ = _cubic_table(tab["z"])
        qF, sF = _cubic_table(tab["F"])
        self._rtab64 = torch.from_numpy(np.stack((qf, qz), axis=1))  # [nr - 1, 2, 4]
        self._ftab64 = torch.from_numpy(qF)                          # [nrho - 1, 4]
        self.rho_max = (self.nrho - 1) * self.drho
        self.f_end = float(tab["F"][-1])
        self.fp_end = float(sF[-1] / self.drho)
        self._tabs_on = {}
        self._nparticles = nparticles
        if pos_dir is not None:
            self.traj = _load_traj(pos_dir).to(device)

    # ------------------------------------------------------------------ tables
    def _tabs(self, device, dtype):
        key = (torch.device(device), dtype)
        if key not in self._tabs_on:
            self._tabs_on[key] = (self._rtab64.to(device=device, dtype=dtype).contiguous(),
                                  self._ftab64.to(device=device, dtype=dtype).contiguous())
        return self._tabs_on[key]

    def _kw(self, device):
        rtab, ftab = self._tabs(device, torch.float32)
        return dict(rtab=rtab, ftab=ftab, dr=self.dr, drho=self.drho, f_end=self.f_end, fp_end=self.fp_end,
                    box=self.box, rc=self.rc)

    def _kernel_ok(self, pos):
        return (self.use_kernels and torch.is_tensor(pos) and pos.is_cuda and pos.dtype == torch.float32
                and pos.dim() >= 2 and pos.shape[-1] == 3 and K_.eam_supported(pos.shape[-2]))

    # ------------------------------------------------------------------ energy
    def potential(self, pos):
        if pos.dim() < 2 or pos.shape[-1] != 3:
            raise ValueError("EAM positions are [..., n, 3]; got shape %s" % (tuple(pos.shape),))
        n = pos.shape[-2]
        if self._kernel_ok(pos):
            x = _rows(pos, n * 3)
            if torch.is_grad_enabled() and x.requires_grad:
                out = _EAMFn.apply(x, self, n)
            else:
                out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
                K_.eam_potential(x.detach(), out, n=n, **self._kw(x.device))
            return out.reshape(pos.shape[:-2])
        rows = max(1, self._CHUNK_ELEMS // (n * n))
        if pos.dim() < 3 or pos.shape[:-2].numel() <= rows:
            return self._potential_torch(pos)
        flat = pos.reshape(-1, n, 3)
        out = torch.cat([self._potential_torch(flat[i:i + rows]) for i in range(0, flat.shape[0], rows)])
        return out.reshape(pos.shape[:-2])

    def _embed_torch(self, rho, ftab):
        t = rho * (1.0 / self.drho)
        m = t.detach().floor().clamp(0, self.nrho - 2)
        inside = _cubic(ftab[m.long()], t - m)
        return torch.where(rho < self.rho_max, inside, self.f_end + self.fp_end * (rho - self.rho_max))

    def _potential_torch(self, pos):
        """The definition in pos's dtype: a loop over the image shifts, each one
        [..., n, n] pair terms; autograd gives the exact gradient of the
        interpolated energy (dp/dr = 1/dr inside the table)."""
        rtab, ftab = self._tabs(pos.device, pos.dtype)
        d = pos.unsqueeze(-2) - pos.unsqueeze(-3)  # d[i, j] = x_i - x_j
        comp = [d[..., a] - self.box[a] * torch.round(d[..., a] * (1.0 / self.box[a])) for a in range(3)]
        rho = torch.zeros(pos.shape[:-1], dtype=pos.dtype, device=pos.device)
        pair = torch.zeros_like(rho)
        nx, ny, nz = self.nshift
        inv_dr = 1.0 / self.dr
        for sx in range(-nx, nx + 1):
            dx = comp[0] + sx * self.box[0]
            dx2 = dx * dx
            for sy in range(-ny, ny + 1):
                dy = comp[1] + sy * self.box[1]
                dxy2 = dx2 + dy * dy
                for sz in range(-nz, nz + 1):
                    dz = comp[2] + sz * self.box[2]
                    r2 = dxy2 + dz * dz
                    nonzero = r2 > 0
                    r = torch.sqrt(torch.where(nonzero, r2, torch.ones_like(r2)))
                    ok = nonzero & (r <= self.rc)
                    if not bool(ok.any()):
                        continue
                    r = torch.where(ok, r, torch.full_like(r, self.dr))  # any in-table value: masked below
                    t = r * inv_dr
                    m = t.detach().floor().clamp(max=self.nr - 2)
                    p = (t - m).clamp(max=1.0)
                    q = rtab[m.long()]
                    zero = torch.zeros_like(r)
                    rho = rho + torch.where(ok, _cubic(q[..., 0, :], p), zero).sum(-1)
                    pair = pair + torch.where(ok, _cubic(q[..., 1, :], p) / r, zero).sum(-1)
        return (self._embed_torch(rho, ftab) + 0.5 * pair).sum(-1)

    def force(self, pos):
        """-dU/dx, [..., n, 3]: the backward kernel on the device, autograd
        through the torch path (row chunk by row chunk) elsewhere."""
        n = pos.shape[-2]
        if self._kernel_ok(pos):
            x = _rows(pos.detach(), n * 3)
            gx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
            K_.eam_potential_bwd(x, torch.ones(x.shape[0], dtype=torch.float32, device=x.device), gx, n=n,
                                 **self._kw(x.device))
            return -gx.reshape(pos.shape)
        flat = pos.detach().reshape(-1, n, 3)
        rows = max(1, self._CHUNK_ELEMS // (n * n))
        out = []
        with torch.enable_grad():
            for i in range(0, flat.shape[0], rows):
                x = flat[i:i + rows].clone().requires_grad_()
                u = self._potential_torch(x)
                out.append(-torch.autograd.grad(u, x, torch.ones_like(u))[0])
        return torch.cat(out).reshape(pos.shape)

    def get_force(self, x):
        return self.force(x)

    @property
    def nparticles(self):
        if self._nparticles is not None:
            return self._nparticles
        if self.position is None:
            raise AttributeError("EAM.nparticles needs nparticles=... or a held position")
        return self.position.shape[-2]

    def _dyn_fused_ok(self, x, v):
        # the bits are equal either way: the cap only picks the faster route
        return super()._dyn_fused_ok(x, v) and x.shape[:-2].numel() <= self._FUSED_ROWS_MAX

    def _dyn_rows(self, t):
        return _rows(t, t.shape[-2] * 3)

    def _dyn_pot_shape(self, pot, x):
        return pot.reshape(x.shape[:-2])

    def _trajectory(self, x, v, xo, vo, pot, path_len, dt, sch):
        # the rows are [n*3]: _integrate notes n
        K_.eam_trajectory(x, v, xo, vo, pot, path_len=path_len, dt=dt, scheme=sch, n=self._traj_n,
                          **self._kw(x.device))

    _zero_momentum_default = True

    def _lv_nd(self, x):
        if x.dim() < 2 or x.shape[-1] != 3:
            raise ValueError("EAM positions are [..., n, 3]; got shape %s" % (tuple(x.shape),))
        return tuple(x.shape[-2:])

    def _langevin_launch(self, x, v, xo, vo, pot, nd, **kw):
        K_.eam_langevin(x, v, xo, vo, pot, n=nd[0], **self._kw(x.device), **kw)

    def _hmc_ok(self, x_cur, shape):
        return self.use_kernels and len(shape) >= 2 and shape[-1] == 3 and K_.eam_hmc_supported(shape[-2])

    def _hmc_launch(self, shape, x_cur, *args, **kw):
        K_.eam_hmc_run(x_cur, *args, n=shape[-2], **self._kw(x_cur.device), **kw)

    def _integrate(self, x, v, path_len, dt, sch, keep_force=False):
        if x.dim() < 2 or x.shape[-1] != 3:
            raise ValueError("EAM positions are [..., n, 3]; got shape %s" % (tuple(x.shape),))
        self._traj_n = x.shape[-2]
        return super()._integrate(x, v, path_len, dt, sch, keep_force)


# ---------------------------------------------------------------------------
class Switch:
    """Hamiltonian switching between a normalised reference A and a target B:
    Langevin dynamics at temperature ``kT`` on the mixed reduced potential

        u_lam(x) = (1 - lam) u_A(x) + lam u_B(x),   u_A = -log p_A,  u_B = U_B / kT

    with the switching work accumulated along the way (Frenkel-Ladd /
    Jarzynski-Crooks; ``app.fe_switching`` hands it to BAR).  ``reference`` is
    an ``EinsteinCrystal`` (or any system whose ``potential`` is minus a
    normalised log density), ``target`` an ``LJ``, an ``EAM`` or any system
    with ``potential`` and ``get_force``.  Positions have the target's shape
    ([..., n, dim] for LJ and EAM, [B, W] otherwise).

    ``lam`` is an fp32 schedule indexed by the ABSOLUTE step, ``lam[j]`` for
    ``0 <= j <= total steps``: linear, any other monotone ramp, or constant.
    Per step k, with l0 = lam[step0 + k] and l1 = lam[step0 + k + 1]:

        if l1 != l0:  w = w + (double(l1) - double(l0)) * (double(U_B(x)) * (1 / kT) - double(u_A(x)))
        a = (1 - l1) * kT;  b = l1;  F = a * g_A + b * g_B
        v = v + hb*F;  x = x + hd*v;  v = c1*v + c2*xi;  x = x + hd*v
        g_A = reference.get_force(x);  g_B = target.get_force(x);  F = a * g_A + b * g_B;  v = v + hb*F

    i.e. the work first, at the position before the step, then one BAOAB step
    under l1 with the constants, the noise (tag 0, keyed by seed, absolute step,
    particle, row) and ``zero_momentum`` of ``langevin`` at ``kT``.
    ``zero_momentum`` defaults to False here: the Einstein field pins the centre
    of mass, so its forces do not sum to zero.  Centre-of-mass and finite-size
    corrections of the Einstein-crystal method are out of scope: the work is
    that of the two Hamiltonians as they are given.

    fp32 device tensors with an ``EinsteinCrystal`` reference and an ``LJ`` or
    ``EAM`` target at the kernels' shapes take nfk_switch.hip: chunks of at most
    ``config.LANGEVIN_STEPS_PER_LAUNCH`` steps per launch, no host sync inside a
    run.  Everything else -- CPU, fp64, ``use_kernels`` or ``fused_dynamics``
    off, other pairs of systems -- takes the per-step path: torch ops over the
    two ``get_force`` and the energies, in the input's dtype.  On the device the
    per-step path has the bits of the launch in x, v, the energies and the work
    (its energies are the kernel's own zero-step call, whose u_A row sum runs in
    the kernel's order).  The schedule is read by absolute index, the noise is
    keyed by the absolute step and the work is added to the carried buffer in
    step order, so a run equals, bit for bit, the same run cut into chunks
    (``step0``, ``work``) or split over row blocks (``row_base``)."""

    fused_dynamics = True

    def __init__(self, reference, target, kT=1.0):
        if not kT > 0:
            raise ValueError("Switch needs kT > 0")
        self.reference, self.target, self.kT = reference, target, float(kT)
        self.position = self.velocity = None

    def set_position(self, position):
        self.position = position

    def get_position(self):
        return self.position

    def set_velocity(self, velocity):
        self.velocity = velocity

    def get_velocity(self):
        return self.velocity

    # ------------------------------------------------------------------ shapes and routing
    def _nd(self, x):
        """(particles, dim) of a row of x; ValueError when A and B disagree."""
        sysnd = self.target if hasattr(self.target, "_lv_nd") else self.reference
        n, dim = sysnd._lv_nd(x)
        wa = getattr(self.reference, "width", None)
        if wa is not None and wa != n * dim:
            raise ValueError("the reference holds %d coordinates per configuration, the target %d x %d"
                             % (wa, n, dim))
        return n, dim

    @staticmethod
    def _as(system, x, rows, n, dim):
        """x in the shape ``system`` takes positions in."""
        return x.reshape(rows, n, dim) if isinstance(system, (LJ, EAM)) else x.reshape(rows, n * dim)

    def _kernels_ok(self, x, nd):
        A, B = self.reference, self.target
        n, dim = nd
        if not (isinstance(A, EinsteinCrystal) and isinstance(B, (LJ, EAM)) and x.dim() >= 2):
            return False
        if not (A.natoms == n and A.dim == dim and A._kernel_ok(x) and B._kernel_ok(x)):
            return False
        return B.boxlength is not None

    def _launch_ok(self, x, v, nd):
        return (self._kernels_ok(x, nd) and self.fused_dynamics and self.reference.fused_dynamics
                and self.target.fused_dynamics and torch.is_tensor(v) and v.dtype == x.dtype
                and v.device == x.device)

    def _launch(self, xr, vr, xo, vo, en, lam, nd, **kw):
        A, B = self.reference, self.target
        scale, hld = A._consts()
        kw = dict(kw, kT=self.kT, scale=scale, hld=hld, boxlength_A=A.boxlength)
        if isinstance(B, LJ):
            K_.lj_switch(xr, vr, xo, vo, en, A.centers, lam, n=nd[0], dim=nd[1], **B._kw(), **kw)
        else:
            K_.eam_switch(xr, vr, xo, vo, en, A.centers, lam, n=nd[0], **B._kw(xr.device), **kw)

    # ------------------------------------------------------------------ energies
    def energies(self, x):
        """(u_A [B], U_B [B]) of the configurations x."""
        x = x.detach()
        n, dim = nd = self._nd(x)
        rows = x.numel() // (n * dim)
        if self._kernels_ok(x, nd):
            xr = self.target._dyn_rows(x)
            en = torch.empty(rows, 2, dtype=torch.float32, device=x.device)
            self._launch(xr, xr, torch.empty_like(xr, memory_format=torch.contiguous_format),
                         torch.empty_like(xr, memory_format=torch.contiguous_format), en, None, nd, nsteps=0,
                         consts=(0.0, 0.0, 0.0, 0.0), seed=0)
            return en[:, 0], en[:, 1]
        with torch.no_grad():
            return (self.reference.potential(self._as(self.reference, x, rows, n, dim)).reshape(-1),
                    self.target.potential(self._as(self.target, x, rows, n, dim)).reshape(-1))

    def potential(self, x, lam):
        """u_lam(x) = (1 - lam) u_A + lam U_B / kT, [B]."""
        ua, ub = self.energies(x)
        return (1.0 - lam) * ua + lam * (ub / self.kT)

    def _forces(self, x, rows, n, dim):
        out = []
        for system in (self.reference, self.target):
            xs = self._as(system, x, rows, n, dim)
            if hasattr(system, "_force_detached"):
                g = system._force_detached(xs)
            else:
                with torch.enable_grad():
                    g = system.get_force(xs.detach()).detach()
            out.append(g.reshape(x.shape))
        return out

    # ------------------------------------------------------------------ the run
    def switch(self, lam, nsteps=None, dt=0.005, gamma=10.0, mass=1.0, seed=0, init_pos=None, init_velocity=None,
               record_every=0, zero_momentum=False, step0=0, row_base=0, work=None):
        """``nsteps`` switching steps (default: to the end of ``lam``) from the
        held position and velocity (or ``init_pos`` / ``init_velocity``; a
        missing velocity is drawn as ``langevin`` draws it: sqrt(kT / mass)
        times the tag-1 normals of step ``step0``).  ``work`` (fp64 [B], default
        zeros) is the work carried in; it is not modified.

        Returns (position, work [B] fp64, energies [B, 2] = (u_A, U_B) at the
        final position) and holds the final state; with ``record_every > 0``
        also the frames on ``langevin``'s schedule and their energies
        [F, B, 2].  ``nsteps = 0`` is the energy evaluation."""
        from . import config, rng
        if init_pos is not None:
            self.set_position(init_pos)
        if init_velocity is not None:
            self.set_velocity(init_velocity)
        x = self.position
        lam_t = torch.as_tensor(lam).detach().reshape(-1).to(torch.float32)
        step0, row_base, seed, record_every = int(step0), int(row_base), int(seed), int(record_every)
        nsteps = lam_t.numel() - 1 - step0 if nsteps is None else int(nsteps)
        if nsteps < 0 or record_every < 0 or step0 < 0:
            raise ValueError("nsteps, record_every and step0 must be >= 0 (and lam must reach step0)")
        if nsteps > 0 and step0 + nsteps >= lam_t.numel():
            raise ValueError("the schedule is too short: lam holds %d values, step0 + nsteps = %d needs %d"
                             % (lam_t.numel(), step0 + nsteps, step0 + nsteps + 1))
        if not (dt > 0 and gamma >= 0 and mass > 0):
            raise ValueError("switch needs dt > 0, gamma >= 0 and mass > 0")
        zm, kT = bool(zero_momentum), self.kT
        n, dim = nd = self._nd(x)
        rows = x.numel() // (n * dim)
        c1 = math.exp(-gamma * dt)
        consts = (0.5 * dt / mass, 0.5 * dt, c1, math.sqrt(kT / mass * (1.0 - c1 * c1)))
        vscale = math.sqrt(kT / mass)
        fp32 = x.dtype == torch.float32
        if fp32:
            consts = tuple(float(np.float32(c)) for c in consts)
            vscale = float(np.float32(vscale))
        if self.velocity is None:
            self.velocity = vscale * rng.philox_normal(seed, rows, n, dim, step0, row_base, tag=1, zero_mean=zm,
                                                       device=x.device, dtype=x.dtype).reshape(x.shape)
        v = self.velocity.reshape(x.shape)
        if work is None:
            w = torch.zeros(rows, dtype=torch.float64, device=x.device)
        else:
            w = work.detach().to(device=x.device, dtype=torch.float64).reshape(rows).clone()
        nframes = (step0 + nsteps) // record_every - step0 // record_every if record_every else 0
        if self._launch_ok(x, v, nd):
            xr, vr = self.target._dyn_rows(x).detach(), self.target._dyn_rows(v).detach()
            xo = torch.empty_like(xr, memory_format=torch.contiguous_format)
            vo = torch.empty_like(vr, memory_format=torch.contiguous_format)
            en = torch.empty(rows, 2, dtype=torch.float32, device=xr.device)
            lam_d = lam_t.to(xr.device).contiguous()
            frames = ens = None
            if record_every:
                frames = torch.empty(nframes, rows, n * dim, dtype=torch.float32, device=xr.device)
                ens = torch.empty(nframes, rows, 2, dtype=torch.float32, device=xr.device)
            cap = max(1, int(config.LANGEVIN_STEPS_PER_LAUNCH))
            done = f0 = 0
            while True:
                m, s0 = min(cap, nsteps - done), step0 + done
                fm = (s0 + m) // record_every - s0 // record_every if record_every else 0
                self._launch(xr, vr, xo, vo, en, lam_d, nd, nsteps=m, consts=consts, seed=seed, step0=s0,
                             row_base=row_base, zero_mean=zm, record_every=record_every, work=w,
                             pos_rec=None if frames is None else frames[f0:f0 + fm],
                             en_rec=None if ens is None else ens[f0:f0 + fm])
                done, f0, xr, vr = done + m, f0 + fm, xo, vo
                if done >= nsteps:
                    break
            x, v = xo.reshape(x.shape), vo.reshape(x.shape)
            if frames is not None:
                frames = frames.reshape(nframes, *x.shape)
        else:
            x, v = x.detach(), v.detach()
            hb, hd, c1, c2 = consts
            lam_h = lam_t.cpu().numpy()
            inv_kT = 1.0 / kT
            gA, gB = self._forces(x, rows, n, dim)
            cur = None  # the energies of the current x, once they are known
            frames, ens = [], []
            for k in range(nsteps):
                l0, l1 = lam_h[step0 + k], lam_h[step0 + k + 1]
                if l1 != l0:
                    cur = self.energies(x) if cur is None else cur
                    w = w + (float(l1) - float(l0)) * (cur[1].double() * inv_kT - cur[0].double())
                if fp32:
                    a, b = float((np.float32(1.0) - l1) * np.float32(kT)), float(l1)
                else:
                    a, b = (1.0 - float(l1)) * kT, float(l1)
                xi = rng.philox_normal(seed, rows, n, dim, step0 + k, row_base, tag=0, zero_mean=zm,
                                       device=x.device, dtype=x.dtype).reshape(x.shape)
                v = v + hb * (a * gA + b * gB)
                x = x + hd * v
                v = c1 * v + c2 * xi
                x = x + hd * v
                gA, gB = self._forces(x, rows, n, dim)
                v = v + hb * (a * gA + b * gB)
                cur = None
                if record_every and (step0 + k + 1) % record_every == 0:
                    cur = self.energies(x)
                    frames.append(x)
                    ens.append(torch.stack(cur, dim=-1))
            cur = self.energies(x) if cur is None else cur
            en = torch.stack(cur, dim=-1)
            if record_every:
                frames = torch.stack(frames) if frames else x.new_empty((0,) + tuple(x.shape))
                ens = torch.stack(ens) if ens else en.new_empty((0, rows, 2))
        self.position, self.velocity = x, v
        if record_every:
            return x, w, en, frames, ens
        return x, w, en
