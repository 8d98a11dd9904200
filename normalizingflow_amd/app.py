"""Experiment configs and checkpoints of the reference's applications layer,
restated for the flow path.

* ``get_cfg_defaults`` / ``read_input`` -- the yacs defaults of
  applications/src/config.py:3-69 and the YAML merge of setup.py:84-88, with a
  small attribute-dict node (yacs is not a dependency here).  As with yacs,
  merging a key the defaults do not define raises ``KeyError``.
* ``build_flows`` / ``build_model`` -- the flow construction of
  setup.py:37-63 (RealNVP / NSF_AR / NSF_CL with the reference's tail bound B
  and NSF_CL mask cycle) and the priors of setup.py:17-30: "Normal",
  "EinsteinCrystal" and "GaussianMixture" (systems.py).
* ``build_potential`` -- the target distribution of setup.py:76-80
  (EinsteinCrystal, GaussianMixture, LJ, and Fe as ``systems.EAM`` when
  ``dataset.eam_file`` names a setfl table); LAMMPS itself and SimData are
  out of scope.
* ``reverse_kl`` / ``forward_kl`` -- the losses of setup.py:90-100;
  ``q_matrix`` -- the Q matrix of test.py:33-50 (generate_from_nf, evaluate
  and the target's energies), up to ``Q = torch.stack(...)``;
  ``q_matrix_relaxed`` -- the same through ``relaxation_step``.
* ``fe_estimates`` / ``fe_diff`` -- the free-energy estimates of test.py:55-68
  (BAR and the two exponential averages) over bar.py's batched solver, with
  bootstrap errors, and on request the multistate ``emus`` of test.py:61-63
  with its asymptotic error (mbar.py); Q never leaves its device.
* ``fe_diff_no_training`` -- the prior-against-target driver of test.py:74-88
  over mbar.py's solver.
* ``metropolize`` -- the Metropolis chain over a batch of frames of
  utils.py:82-99, one energy call and one launch (reweight.py);
  ``metropolized_samples`` -- flow samples, their energies and the independence
  sampler over them, with acceptance rates and effective sample sizes.
* ``structure`` -- the radial distribution functions of the flow's samples, of
  the same samples under their importance weights and of the target's samples
  on one grid, with the weights' effective sample size (observables.py).
* ``collect_hmc_data`` / ``integrate_out_v`` / ``relaxation_step`` -- the
  dynamics of applications/src/dynamics.py over systems.py's own integrators
  (no LAMMPS), every trajectory of a call in one launch.
* ``sample_md`` -- target samples by Langevin dynamics at ``dataset.kT``
  (systems.*.langevin), the role of the reference's LAMMPS trajectories.
* ``switching_work`` / ``fe_switching`` / ``fe_stratified`` -- the free energy
  of the target against the (normalised) prior WITHOUT a flow: Hamiltonian
  switching under Langevin dynamics (systems.Switch) with the work handed to
  BAR, and constant-lambda strata handed to MBAR; the check of ``fe_diff``.
* ``save_checkpoint`` / ``load_checkpoint`` -- the checkpoint dict of
  train.py:39-40 and the loader of setup.py:102-109 (``load_state_dict``
  with ``strict=False``), read with ``torch.load(weights_only=True)``.
"""
from __future__ import annotations

import ast
import copy

import torch
import yaml

from . import bar as bar_
from . import flows as F_
from . import mbar as mbar_
from . import observables as observables_
from . import reweight as reweight_
from . import systems
from .hmc import HMC
from .models import NormalizingFlowModel

__all__ = ["CfgNode", "get_cfg_defaults", "read_input", "tail_bound", "build_flows", "build_prior",
           "build_potential", "build_model", "save_checkpoint", "load_checkpoint", "train_step",
           "reverse_kl", "forward_kl", "generate_from_nf", "evaluate", "q_matrix", "collect_hmc_data",
           "integrate_out_v", "relaxation_step", "q_matrix_relaxed", "fe_estimates", "fe_diff",
           "fe_diff_no_training", "metropolize", "metropolized_samples", "structure", "sample_md",
           "switching_work", "fe_switching", "fe_stratified"]


class CfgNode(dict):
    """Nested attribute dictionary with yacs-style ``merge_from_file``."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v

    def clone(self):
        return copy.deepcopy(self)

    def merge_from_dict(self, d, path=""):
        for k, v in d.items():
            if k not in self:
                raise KeyError("Non-existent config key: %s%s" % (path, k))
            if isinstance(self[k], CfgNode):
                if not isinstance(v, dict):
                    raise ValueError("config key %s%s must be a mapping" % (path, k))
                self[k].merge_from_dict(v, path + k + ".")
            else:
                self[k] = _decode(v)

    def merge_from_file(self, filename):
        with open(filename) as f:
            self.merge_from_dict(yaml.safe_load(f) or {})


def _decode(v):
    """yacs decodes string values with ast.literal_eval ("5e-3" -> 0.005; YAML
    itself reads an exponent without a dot as a string)."""
    if isinstance(v, str):
        try:
            return ast.literal_eval(v)
        except (ValueError, SyntaxError):
            return v
    return v


def _node(**kw):
    n = CfgNode()
    for k, v in kw.items():
        n[k] = v
    return n


def get_cfg_defaults():
    """applications/src/config.py:3-69."""
    dataset = _node(name=None, potential=None, training_data=None, testing_data=None, data=None,
                    nparticles=32, dim=3, kT=1.0, rho=None, ncellx=None, ncelly=None, ncellz=None,
                    cell_len=None, boxlength=None, periodic=True, type="xyz", sigma=1.0,
                    epsilon=1.0, cutoff=1.6, shift=True, centers=None, vars=None, alpha=None,
                    input_dir=None, eam_file=None)
    return _node(
        device="cuda:0",
        dataset=dataset,
        flow=_node(type="NSF_AR", nlayers=3, nsplines=32, hidden_dim=100),
        # prior.nparticles/dim/boxlength are copies of the dataset defaults (config.py:48-50)
        prior=_node(type=None, lattice_dir=None, alpha=100, centers=None, vars=None,
                    nparticles=32, dim=3, boxlength=None),
        train_parameters=_node(max_epochs=4000, batch_size=100, output_freq=100,
                               learning_rate=1e-4, scheduler="exponential",
                               lr_scheduler_gamma=0.999),
        output=_node(training_dir="../training/", testing_dir="../testing/",
                     model_dir="../saved_models/", best_model_dir="../trained_models/"))


def read_input(path):
    """setup.py:84-88 (without the print)."""
    cfg = get_cfg_defaults()
    cfg.merge_from_file(path)
    return cfg


def tail_bound(cfg):
    """The spline tail bound B of setup.py:38-44 (None when the config sets
    neither rho nor ncellx; the reference then fails only if it needs B)."""
    d = cfg.dataset
    if d.rho is not None:
        return (d.nparticles / (8 * d.rho)) ** (1 / 3)
    if d.ncellx is not None:
        return d.ncellx * d.cell_len / 2
    return None


def build_flows(cfg):
    """setup.py:55-62."""
    N = cfg.dataset.nparticles * cfg.dataset.dim
    fl = cfg.flow
    B = tail_bound(cfg)
    if fl.type == "RealNVP":
        return [F_.RealNVP(dim=N, hidden_dim=fl.hidden_dim) for _ in range(fl.nlayers)]
    if B is None:
        raise NameError("name 'B' is not defined (set dataset.rho or dataset.ncellx)")
    if fl.type == "NSF_AR":
        return [F_.NSF_AR(dim=N, K=fl.nsplines, B=B, hidden_dim=fl.hidden_dim, device=cfg.device)
                for _ in range(fl.nlayers)]
    if fl.type == "NSF_CL":
        cycle = [[0], [1], [2], [0, 1], [1, 2], [0, 2]]
        masks = sum([cycle for _ in range(fl.nlayers // 6 + 1)], [])[:fl.nlayers]
        return [F_.NSF_CL(size=cfg.dataset.nparticles, dim=3, K=fl.nsplines, B=B,
                          hidden_dim=fl.hidden_dim, mask=masks[i], device=cfg.device)
                for i in range(fl.nlayers)]
    raise ValueError("flow type %r is not built by setup.py" % fl.type)


def _parse_potential(name, c, device, what):
    """setup.py:17-36 for the distributions this package builds."""
    if name == "GaussianMixture":
        return systems.GaussianMixture(c.centers, c.vars, c.nparticles, c.dim, device=device)
    if name == "EinsteinCrystal":
        return systems.EinsteinCrystal(c.centers, c.dim, boxlength=c.boxlength, alpha=c.alpha, device=device)
    if name == "Normal":
        N = c.nparticles * c.dim
        var = 1 if c.vars is None else c.vars
        return torch.distributions.MultivariateNormal(torch.zeros(N, device=device),
                                                      var * torch.eye(N, device=device))
    if name == "LJ" and what == "potential":
        return systems.LJ(pos_dir=c.data, boxlength=c.boxlength, device=device, sigma=c.sigma,
                          epsilon=c.epsilon, cutoff=c.cutoff, shift=c.shift)
    if name == "Fe" and what == "potential" and c.eam_file is not None:
        # the reference's LAMMPS input (input_dir) is not read: the setfl table is the model
        box = tuple(nc * c.cell_len for nc in (c.ncellx, c.ncelly, c.ncellz))
        return systems.EAM(c.eam_file, box, nparticles=c.nparticles, pos_dir=c.data, device=device)
    raise NotImplementedError("%s %r is not built here (systems.py holds EinsteinCrystal, GaussianMixture, "
                              "LJ and EAM; potential 'Fe' needs dataset.eam_file, a setfl table, and is no "
                              "prior; LAMMPS itself and SimData are out of scope); pass an object instead"
                              % (what, name))


def build_prior(cfg, device):
    """The "Normal", "EinsteinCrystal" and "GaussianMixture" priors of
    setup.py:17-30 from ``cfg.prior``."""
    if cfg.prior.type == "LJ":
        raise NotImplementedError("prior 'LJ' has no log_prob; pass a prior object to build_model")
    return _parse_potential(cfg.prior.type, cfg.prior, device, "prior")


def build_potential(cfg, mode="training", device=None):
    """The target of setup.py:76-80: ``cfg.dataset.data`` is set from
    training_data / testing_data by ``mode``, then ``cfg.dataset.potential``
    (EinsteinCrystal, GaussianMixture, LJ, Normal, or Fe with
    ``dataset.eam_file``: ``systems.EAM`` in the box ``(ncellx, ncelly,
    ncellz) * cell_len``) is built from ``cfg.dataset``.  As in setup_model, a
    missing ``dataset.boxlength`` becomes 2 B first."""
    device = cfg.device if device is None else device
    if cfg.dataset.boxlength is None and tail_bound(cfg) is not None:
        cfg.dataset.boxlength = 2 * tail_bound(cfg)
    if mode == "training":
        cfg.dataset.data = cfg.dataset.training_data
    elif mode == "testing":
        cfg.dataset.data = cfg.dataset.testing_data
    return _parse_potential(cfg.dataset.potential, cfg.dataset, device, "potential")


def build_model(cfg, prior=None, device=None):
    """NormalizingFlowModel(prior, flows, cfg.device).to(device) (setup.py:63)."""
    device = cfg.device if device is None else device
    prior = build_prior(cfg, device) if prior is None else prior
    if cfg.dataset.boxlength is None and tail_bound(cfg) is not None:
        cfg.dataset.boxlength = 2 * tail_bound(cfg)
    return NormalizingFlowModel(prior, build_flows(cfg), device).to(device)


def save_checkpoint(path, model, optimizer=None, scheduler=None, epoch=0, losses=()):
    """train.py:39-40: {"model", "optim", "scheduler", "epoch", "loss"}."""
    torch.save({"model": model.state_dict(),
                "optim": None if optimizer is None else optimizer.state_dict(),
                "scheduler": None if scheduler is None else scheduler.state_dict(),
                "epoch": epoch,
                "loss": [float(v) for v in losses]}, path)


def load_checkpoint(model, path, optimizer=None, scheduler=None):
    """setup.py:102-109: load the "model" entry with strict=False (weights only;
    nothing in the file is executed).  Returns the checkpoint dict."""
    ck = torch.load(path, map_location="cpu", weights_only=True)
    model.load_state_dict(ck["model"], strict=False)
    if optimizer is not None and ck.get("optim") is not None:
        optimizer.load_state_dict(ck["optim"])
    if scheduler is not None and ck.get("scheduler") is not None:
        scheduler.load_state_dict(ck["scheduler"])
    return ck


def train_step(model, optimizer, x, scheduler=None):
    """One iteration of train.py:21-29: forward KL / NLL, backward, step."""
    optimizer.zero_grad()
    z, prior_logprob, log_det = model(x)
    loss = -torch.mean(prior_logprob + log_det)
    loss.backward()
    optimizer.step()
    if scheduler is not None:
        scheduler.step()
    return loss.detach()


def reverse_kl(model, potential, nsamples):
    """setup.py:90-94 (reverseKL): prior samples pushed through the inverse
    flow, scored by the target."""
    z = model.prior.sample((nsamples,))
    x, log_det = model.inverse(z)
    log_prob = model.prior.log_prob(z) - log_det
    return -torch.mean(potential.log_prob(x)) + torch.mean(log_prob)


def forward_kl(model, potential, nsamples):
    """setup.py:96-100 (KL): target samples scored by the flow."""
    x = potential.sample(nsamples, flatten=True)
    z, prior_logprob, log_det = model(x)
    logprob = prior_logprob + log_det
    return -torch.mean(logprob) + torch.mean(potential.log_prob(x))


def generate_from_nf(model, nsamples=50, batchsize=50):
    """test.py:13-22: nsamples // batchsize batches of model.sample."""
    xs, lps = [], []
    for _ in range(nsamples // batchsize):
        x, log_px, _ = model.sample(batchsize)
        xs.append(x)
        lps.append(log_px)
    return torch.cat(xs, dim=0), torch.cat(lps, dim=0)


def evaluate(model, x, batchsize=50):
    """test.py:24-31: model.evaluate over len(x) // batchsize batches."""
    return torch.cat([model.evaluate(x[i * batchsize:(i + 1) * batchsize])
                      for i in range(len(x) // batchsize)], dim=0)


def q_matrix(cfg, model, potential, nsamples, batchsize=500):
    """The [2, nsamples, 2] tensor Q of test.py:34-50 without relaxation:
    Q[0] = (log q, -U/kT) of flow samples, Q[1] = the same of target samples.
    The energies stay on the device and nothing is written; ``fe_estimates``
    turns Q into free-energy estimates."""
    d = cfg.dataset
    traj0, q00 = generate_from_nf(model, nsamples, batchsize=batchsize)
    q01 = -(potential.potential(traj0.reshape(-1, d.nparticles, d.dim)) / d.kT).detach().to(q00.device)
    Q0 = torch.transpose(torch.vstack((q00, q01)), 0, 1)
    traj1 = potential.sample(nsamples)
    traj1 = traj1.reshape(len(traj1), -1).to(q00.device)
    q10 = torch.zeros(nsamples, device=q00.device)
    q10 += evaluate(model, traj1, batchsize=batchsize)
    q11 = -(potential.potential(traj1.reshape(-1, d.nparticles, d.dim)) / d.kT).detach().to(q00.device)
    Q1 = torch.transpose(torch.vstack((q10, q11)), 0, 1)
    return torch.stack((Q0, Q1))


def _sim_positions(simulation, rows, dim):
    """[B, W] rows in the shape the simulation holds positions in (LJ, EAM: [B, n, dim])."""
    if isinstance(simulation, (systems.LJ, systems.EAM)):
        return rows.reshape(rows.shape[0], -1, dim)
    return rows


def collect_hmc_data(cfg, model, hmc, burnin=100, epochs=500, one_launch=False):
    """dynamics.py:59-65 without the file writes: one model sample relaxed by
    ``epochs`` HMC moves; returns (traj[burnin:], acceptance rate).
    ``one_launch=True`` runs the epochs in one launch (``HMC.hmc``)."""
    samples, _, _ = model.sample(1)
    init = _sim_positions(hmc.simulation, samples.detach().reshape(1, -1), hmc.dim)[0]
    if one_launch:
        traj, _, _, acc_prob = hmc.hmc(epochs=epochs, init_pos=init, one_launch=True)
    else:
        traj, _, _, acc_prob = hmc.hmc(epochs=epochs, init_pos=init)
    return traj[burnin:], acc_prob


def integrate_out_v(model, hmc, frames, npoints=10):
    """dynamics.py:26-36 for every row of ``frames`` [F, W] at once: npoints
    velocity draws per frame, all F * npoints trajectories in one launch, one
    ``model.evaluate``, then logsumexp over a frame's draws - log(npoints): [F]
    (a 1-D frame gives a scalar, as the reference does)."""
    rows = frames.detach().reshape(1, -1) if frames.dim() == 1 else frames.detach().reshape(len(frames), -1)
    start = rows.repeat_interleave(npoints, dim=0)  # frame-major: a frame's draws are consecutive
    hmc.simulation.set_position(_sim_positions(hmc.simulation, start, hmc.dim))
    v, _ = hmc.generate_v()
    position, _, _ = hmc.run_sim(v)
    q_nf = model.evaluate(position.reshape(start.shape).float())
    out = torch.logsumexp(q_nf.reshape(rows.shape[0], npoints), 1) - torch.log(torch.tensor(float(npoints)))
    return out[0] if frames.dim() == 1 else out


def relaxation_step(cfg, model, simulation, traj, path_len=12, beta=None, init_beta=None, mass=None,
                    npoints=10):
    """dynamics.py:38-56 in its generic form (``simulation`` is one of
    systems.py's classes): one HMC trajectory of ``path_len`` steps per row of
    ``traj``, all in one launch, then ``integrate_out_v`` of the relaxed frames.
    Returns (traj_new, q_learned, -U_new / kT) on ``cfg.device``.  ``beta``
    defaults to 1 / cfg.dataset.kT."""
    kT = cfg.dataset.kT
    run = HMC(simulation, beta=1 / kT if beta is None else beta, mass=mass, path_len=path_len,
              init_beta=init_beta, dim=cfg.dataset.dim)
    rows = traj.detach().reshape(len(traj), -1)
    simulation.set_position(_sim_positions(simulation, rows, cfg.dataset.dim))
    position, potential, _ = run.run_sim()
    traj_new = position.reshape(rows.shape)
    q_learned = integrate_out_v(model, run, traj_new, npoints)
    return (traj_new.float().to(cfg.device), q_learned.to(cfg.device),
            (-potential.reshape(-1) / kT).to(cfg.device))


def q_matrix_relaxed(cfg, model, potential, nsamples, batchsize=500, **relaxation_kw):
    """The Q of test.py:34-50 with ``relaxation=True``: the flow's samples and
    the target's each go through ``relaxation_step`` (test.py:35-36, 41-42),
    whose keyword arguments ``relaxation_kw`` are."""
    traj0, _ = generate_from_nf(model, nsamples, batchsize=batchsize)
    _, q00, q01 = relaxation_step(cfg, model, potential, traj0, **relaxation_kw)
    traj1 = potential.sample(nsamples)
    _, q10, q11 = relaxation_step(cfg, model, potential, traj1, **relaxation_kw)
    Q0 = torch.transpose(torch.vstack((q00, q01)), 0, 1)
    Q1 = torch.transpose(torch.vstack((q10, q11)), 0, 1)
    return torch.stack((Q0, Q1)).detach()


def fe_estimates(cfg, Q, nboot=0, generator=None, emus=False):
    """test.py:55-68 from a [2, N, 2] Q on any device: the offsets
    ``to_subtract_0/1`` (the minima of Q[1]'s columns), the work values
    ``w_F = Q[0,:,0] - Q[0,:,1]`` and ``w_R = -Q[1,:,0] + Q[1,:,1]`` of the
    shifted Q in Q's dtype, and with off = to_subtract_0 - to_subtract_1

        bar = (off + DeltaF) / nparticles * kT      (DeltaF: bar.BAR(w_F, w_R))
        md  = (off - log mean exp(w_R)) / nparticles * kT
        nf  = (off + log mean exp(w_F)) / nparticles * kT

    as 0-d fp64 tensors on Q's device; nothing synchronises.  With ``nboot`` > 0
    the bootstrap standard deviations ``(bar_err, md_err, nf_err)`` follow
    (``nboot`` resamples of w_F and w_R, ``bar.bootstrap``).  Q is not modified
    (the reference shifts it in place).

    ``emus=True`` appends the multistate estimate of test.py:61-63 to the
    estimates, ``(bar, md, nf, emus)`` as test.py:72 returns them:

        emus = (off + f_1 - f_0) / nparticles * kT   (f: mbar.mbar_solve(-Q))

    with ``log c_0 - log c_1 = f_1 - f_0`` for the normalising constants
    ``c = exp(-f)`` of ``MBAR(-Q).norm_const()``, from one solve on the shifted
    Q run to convergence (the reference caps its plain iteration at 40).  With
    ``nboot`` > 0 as well the errors follow as ``(bar_err, md_err, nf_err,
    emus_err)``; ``emus_err`` is the asymptotic standard deviation of f_1 - f_0
    from the same solve's Gram matrix (``mbar.mbar_std``), scaled like emus, in
    place of the private solver's error of test.py:70."""
    d = cfg.dataset
    Q = Q.detach()
    if Q.dim() != 3 or Q.shape[0] != 2 or Q.shape[2] != 2:
        raise ValueError("Q must be [2, N, 2], got %s" % (tuple(Q.shape),))
    to_subtract = torch.stack((torch.min(Q[1][:, 0]), torch.min(Q[1][:, 1])))
    Qs = Q - to_subtract
    w_F = Qs[0][:, 0] - Qs[0][:, 1]
    w_R = -Qs[1][:, 0] + Qs[1][:, 1]
    off = (to_subtract[0] - to_subtract[1]).double()

    def scaled(o):
        return tuple((off + sgn * o[..., j]) / d.nparticles * d.kT for j, sgn in ((0, 1.0), (2, -1.0), (1, 1.0)))

    out, _ = bar_.bar_solve(w_F, w_R)
    est = scaled(out[0])
    if emus:
        n_k = [Q.shape[1]] * 2
        f, _, gram = mbar_.mbar_solve((-Qs).reshape(-1, 2), n_k)
        est = est + ((off + (f[0, 1] - f[0, 0])) / d.nparticles * d.kT,)
    if not nboot:
        return est
    boot = scaled(bar_.bootstrap(w_F, w_R, nboot, generator=generator))
    err = tuple(b.std() for b in boot)
    if emus:
        err = err + (mbar_.mbar_std(gram, n_k, 0, 1)[0] / d.nparticles * d.kT,)
    return est + err


def fe_diff(cfg, model, potential, nsamples, relaxation=False, return_err=False, nboot=200, batchsize=500,
            *, generator=None, relaxation_kw=None, emus=False):
    """test.py:33-72: ``(bar, md, nf)`` free-energy differences per particle
    between the flow and its target from ``nsamples`` samples of each
    (``relaxation=True``: both relaxed by ``relaxation_step`` first, called with
    ``relaxation_kw``).  ``return_err=True`` appends the bootstrap standard
    deviations ``(bar_err, md_err, nf_err)`` over ``nboot`` resamples.  Every
    result is a 0-d fp64 tensor on the model's device.  No file is written and
    nothing is plotted.  ``emus=True`` appends the multistate estimate of
    test.py:61-63 to the estimates and, with ``return_err=True``, its asymptotic
    standard deviation to the errors (see ``fe_estimates``)."""
    if relaxation:
        Q = q_matrix_relaxed(cfg, model, potential, nsamples, batchsize=batchsize, **(relaxation_kw or {}))
    else:
        Q = q_matrix(cfg, model, potential, nsamples, batchsize=batchsize)
    return fe_estimates(cfg, Q, nboot=nboot if return_err else 0, generator=generator, emus=emus)


def metropolize(cfg, potential, x, burnin=20, *, log_q=None, generator=None, return_chain=False):
    """utils.py:82-99: the Metropolis chain whose proposal at step i is frame i
    of ``x`` (N frames of ``nparticles * dim`` coordinates).  All N energies come
    from one ``potential.potential`` call, the uniforms from one ``torch.rand(N,
    generator=generator)`` on x's device, and the chain is one launch
    (``reweight.metropolis_chain``); nothing is moved to the host.

    Returns the reference's pair: ``x[index]`` ([M, nparticles, dim]), where
    ``index[i]`` is true where step i accepted and ``i > burnin``, and the reduced
    energies U/kT of every accepted step, burn-in included, as a tensor (the
    reference returns a list).

    With ``log_q=None`` the test is the reference's, ``r < exp(U_cur/kT -
    U_i/kT)``, on the energy alone: it samples the target only if the frames
    were proposed uniformly, which samples of a flow are not.  With ``log_q``,
    the flow's log density of every frame ([N]), it is the independence sampler
    ``r < exp((U_cur/kT + log q_cur) - (U_i/kT + log q_i))``, whose stationary
    distribution is the target.

    ``return_chain=True`` returns ``(x[state[burnin+1:]], e[state[burnin+1:]],
    acceptance rate)`` instead: the chain's state after every step past the
    burn-in, repeats included, its reduced energies, and naccept / N as a 0-d
    tensor.  The shapes are fixed and nothing here synchronises (the potential's
    own NaN check follows ``config.STRICT_CHECKS``), so the call can be captured
    in a graph."""
    d = cfg.dataset
    frames = x.detach().reshape(-1, d.nparticles, d.dim)
    e = (potential.potential(frames) / d.kT).detach().reshape(-1).to(frames.device)
    N = e.numel()
    r = torch.rand(N, generator=generator, device=frames.device).to(e.dtype)
    lq = None if log_q is None else log_q.detach().reshape(-1).to(e.device)
    state, accepted, naccept, _ = reweight_.metropolis_chain(e, r, lq)
    if return_chain:
        kept = state[burnin + 1:].long()
        return frames[kept], e[kept], naccept.double() / max(N, 1)
    index = accepted.clone()
    index[:burnin + 1] = False
    return frames[index], e[accepted]


def metropolized_samples(cfg, model, potential, nsamples, batchsize=500, chains=1, burnin=0, generator=None):
    """Samples of the target from the flow: ``chains * nsamples`` flow samples
    with their log q (``generate_from_nf``; the product must be a multiple of
    ``batchsize``), their energies in one ``potential.potential`` call, and
    ``chains`` independence-sampler chains over ``nsamples`` proposals each in one
    launch (the correct rule of ``metropolize``, uniforms from one ``torch.rand``
    through ``generator``).  Returns ``(x_chain [chains, nsamples - burnin, W],
    acceptance [chains], ess [chains])``: every chain's states from step
    ``burnin`` on, its acceptance rate over all steps, and the Kish effective
    sample size of its proposals' importance weights (``reweight.ess``), both
    fp64.  The chain and the weights do not synchronise."""
    d = cfg.dataset
    total = chains * nsamples
    if total < 1 or total % batchsize:
        raise ValueError("chains * nsamples = %d must be a positive multiple of batchsize %d" % (total, batchsize))
    with torch.no_grad():
        x, log_q = generate_from_nf(model, total, batchsize=batchsize)
    x, log_q = x.detach(), log_q.detach().reshape(chains, nsamples)
    e = (potential.potential(x.reshape(-1, d.nparticles, d.dim)) / d.kT).detach().to(x.device)
    e = e.reshape(chains, nsamples)
    r = torch.rand(chains, nsamples, generator=generator, device=x.device).to(e.dtype)
    state, _, naccept, _ = reweight_.metropolis_chain(e, r, log_q.to(e.dtype))
    rows = x.reshape(chains, nsamples, -1)
    kept = state[:, burnin:].long().unsqueeze(-1).expand(-1, -1, rows.shape[-1])
    return (torch.gather(rows, 1, kept), naccept.double() / nsamples,
            reweight_.ess(reweight_.log_weights(log_q, e)))


def structure(cfg, model, potential, nsamples, batchsize=500, nbins=100, r_max=None):
    """The structure of the flow's samples against the target's, as radial
    distribution functions on one grid (``observables.rdf``): ``nsamples`` flow
    samples with their log q (``generate_from_nf``, as ``q_matrix`` draws them)
    and their energies over kT in one ``potential.potential`` call, and
    ``potential.sample(nsamples)``.  Returns a dict:

        r             bin centres [nbins]
        g_flow        g(r) of the flow's samples as drawn
        g_reweighted  g(r) of the same samples under their importance weights
                      (``reweight.log_weights``, self-normalised)
        g_target      g(r) of the target's samples
        ess           the Kish effective sample size of those weights (0-d)

    all fp64 on the model's device.  The box is ``potential.boxlength`` (a scalar
    or one length per dimension), else ``cfg.dataset.boxlength``; ``r_max=None``
    is half its shortest length.  Nothing leaves the device and nothing is
    written."""
    d = cfg.dataset
    box = getattr(potential, "boxlength", None)
    if box is None:
        box = d.boxlength
    with torch.no_grad():
        x, log_q = generate_from_nf(model, nsamples, batchsize=batchsize)
    x, log_q = x.detach().reshape(-1, d.nparticles, d.dim), log_q.detach()
    e = (potential.potential(x) / d.kT).detach().reshape(-1).to(x.device)
    logw = reweight_.log_weights(log_q.to(e.dtype), e)
    target = potential.sample(nsamples)
    target = target.reshape(len(target), d.nparticles, d.dim).to(x.device)
    r, g_flow = observables_.rdf(x, box, r_max=r_max, nbins=nbins)
    _, g_rew = observables_.rdf(x, box, r_max=r_max, nbins=nbins, log_weights=logw)
    _, g_target = observables_.rdf(target, box, r_max=r_max, nbins=nbins)
    return {"r": r, "g_flow": g_flow, "g_reweighted": g_rew, "g_target": g_target, "ess": reweight_.ess(logw)}


def sample_md(cfg, potential, nsamples, x0=None, chains=16, burnin=1000, stride=50, dt=0.005, gamma=10.0, seed=0):
    """Target samples by Langevin dynamics at ``cfg.dataset.kT`` (the role of the
    reference's LAMMPS runs with ``integrator="langevin"``, systems.py:25-26):
    ``chains`` independent chains of ``potential.langevin`` from ``x0``
    ([nparticles, dim] for every chain, or [chains, nparticles, dim]; default:
    the centres of the Einstein-crystal prior when ``cfg.prior.type`` is
    "EinsteinCrystal"), ``burnin`` steps, then one frame of every chain each
    ``stride`` steps until there are ``nsamples``.  Returns
    [nsamples, nparticles, dim], what ``potential.update_data`` accepts; frames
    of one time are adjacent.  The run is a function of ``seed`` alone.  The
    chains are left in ``potential``'s held position and velocity."""
    d = cfg.dataset
    nsamples, chains = int(nsamples), max(1, min(int(chains), int(nsamples)))
    device = getattr(potential, "device", cfg.device)
    if x0 is None:
        if cfg.prior.type != "EinsteinCrystal":
            raise ValueError("sample_md needs x0 unless cfg.prior.type is 'EinsteinCrystal' (whose centres start "
                             "the chains)")
        x0 = systems._centers(cfg.prior.centers if cfg.prior.centers is not None else cfg.prior.lattice_dir,
                              cfg.prior.dim, device)
    x0 = torch.as_tensor(x0, dtype=torch.float32).to(device)
    n, dim = x0.shape[-2:]
    x0 = x0.expand(chains, n, dim).contiguous() if x0.dim() == 2 else x0
    if x0.shape[0] != chains:
        raise ValueError("x0 holds %d chains, chains=%d" % (x0.shape[0], chains))
    per = -(-nsamples // chains)
    if not isinstance(potential, (systems.LJ, systems.EAM)):
        x0 = x0.reshape(chains, n * dim)
    kw = dict(dt=dt, gamma=gamma, kT=d.kT, seed=seed)
    potential.set_velocity(None)
    potential.langevin(int(burnin), init_pos=x0, **kw)
    frames = potential.langevin(per * int(stride), record_every=int(stride), step0=int(burnin), **kw)[2]
    return frames.reshape(-1, n, dim)[:nsamples]


def _switch_for(cfg, prior, potential):
    """``systems.Switch(prior, potential, kT)`` after the checks of the switching drivers."""
    d = cfg.dataset
    if not hasattr(prior, "log_prob"):
        raise ValueError("the reference of a switching run must be a normalised density (a prior with log_prob, "
                         "e.g. EinsteinCrystal); got %s" % type(prior).__name__)
    width = getattr(prior, "width", None)
    if width is not None and width != d.nparticles * d.dim:
        raise ValueError("the reference holds %d coordinates, the config %d particles x %d"
                         % (width, d.nparticles, d.dim))
    return systems.Switch(prior, potential, kT=d.kT)


def _ramp(schedule, nsteps):
    """The ramp 0 -> 1 over ``nsteps`` steps as nsteps + 1 fp32 values."""
    if nsteps < 1:
        raise ValueError("a switching run needs nsteps >= 1")
    if isinstance(schedule, str):
        if schedule != "linear":
            raise ValueError("schedule must be 'linear' or the nsteps + 1 values of a ramp from 0 to 1")
        return (torch.arange(nsteps + 1, dtype=torch.float64) / nsteps).float()
    ramp = torch.as_tensor(schedule, dtype=torch.float32).reshape(-1).cpu()
    if ramp.numel() != nsteps + 1:
        raise ValueError("the schedule is too short or too long: %d values for nsteps = %d (needs nsteps + 1)"
                         % (ramp.numel(), nsteps))
    return ramp


def switching_work(cfg, prior, potential, nsamples, nsteps, direction="forward", equil=0, schedule="linear",
                   dt=0.005, gamma=10.0, seed=0, x0=None):
    """The reduced work of ``nsamples`` independent switching trajectories between
    the normalised ``prior`` (lam = 0) and ``potential`` (lam = 1) at
    ``cfg.dataset.kT`` (``systems.Switch``), [nsamples] fp64 on the samples'
    device.  ``direction="forward"``: ``prior.sample(nsamples)``, ``equil`` steps
    at lam = 0, then lam from 0 to 1 over ``nsteps`` steps.  ``"reverse"``:
    ``potential.sample(nsamples)`` (or ``x0``), ``equil`` steps at lam = 1, then
    1 to 0.  ``schedule`` is "linear" or the nsteps + 1 values of a ramp from 0
    to 1 (walked backwards in reverse).  The signs are those of
    ``fe_estimates``' ``w_F`` / ``w_R``: with ``nsteps = 1`` the forward work is
    u_B - u_A at the prior's samples, the reverse work u_A - u_B at the
    target's.  The run is a function of ``seed`` and the starting samples."""
    d = cfg.dataset
    if direction not in ("forward", "reverse"):
        raise ValueError("direction must be 'forward' or 'reverse', got %r" % (direction,))
    sw = _switch_for(cfg, prior, potential)
    nsteps, equil = int(nsteps), int(equil)
    if equil < 0:
        raise ValueError("equil must be >= 0")
    ramp = _ramp(schedule, nsteps)
    if direction == "forward":
        x = prior.sample(nsamples)
        lam = torch.cat((torch.zeros(equil), ramp))
    else:
        x = potential.sample(nsamples) if x0 is None else x0
        lam = torch.cat((torch.ones(equil), ramp.flip(0)))
    x = _sim_positions(potential, x.detach().reshape(len(x), -1), d.dim)
    sw.set_velocity(None)
    return sw.switch(lam, dt=dt, gamma=gamma, seed=seed, init_pos=x)[1]


def fe_switching(cfg, prior, potential, nsamples, nsteps, nboot=0, generator=None, **kw):
    """The free-energy difference per particle between ``prior`` and
    ``potential`` WITHOUT a flow: ``nsamples`` forward and ``nsamples`` reverse
    switching trajectories of ``nsteps`` steps (``switching_work``, whose other
    keyword arguments ``kw`` are; the reverse run takes ``seed + 1``), and their
    work values through ``bar.bar_solve``.  Returns ``(bar, md, nf)`` in the
    units and layout of ``fe_estimates`` (its formulas with a zero offset:
    ``bar = DeltaF / nparticles * kT``, ``nf`` the forward exponential average
    ``log mean exp(w_F)`` and ``md`` the reverse one ``-log mean exp(w_R)``, scaled
    alike), and with ``nboot`` > 0 the bootstrap standard deviations ``(bar_err,
    md_err, nf_err)`` (``bar.bootstrap``), all 0-d fp64 tensors on the samples'
    device.  With the flow's prior as ``prior`` the result is directly
    comparable with ``fe_diff(cfg, model, potential, ...)``: both estimate
    -kT / N ln Z_target, this one from the dynamics alone.  On the device the
    work values go to the BAR kernel in fp32."""
    d = cfg.dataset
    seed, x0 = int(kw.pop("seed", 0)), kw.pop("x0", None)
    w_F = switching_work(cfg, prior, potential, nsamples, nsteps, direction="forward", seed=seed, **kw)
    w_R = switching_work(cfg, prior, potential, nsamples, nsteps, direction="reverse", seed=seed + 1, x0=x0, **kw)
    if w_F.is_cuda:
        w_F, w_R = w_F.float(), w_R.float()

    def scaled(o):
        return tuple(sgn * o[..., j] / d.nparticles * d.kT for j, sgn in ((0, 1.0), (2, -1.0), (1, 1.0)))

    est = scaled(bar_.bar_solve(w_F, w_R)[0][0])
    if not nboot:
        return est
    boot = scaled(bar_.bootstrap(w_F, w_R, nboot, generator=generator))
    return est + tuple(b.std() for b in boot)


def fe_stratified(cfg, prior, potential, lambdas, nsamples, equil, stride, chains=16, dt=0.005, gamma=10.0,
                  seed=0, x0=None):
    """The same difference by stratification: one constant-lam run of
    ``systems.Switch`` per value of ``lambdas`` (2 <= K <= 8, the states of the
    MBAR launch; the first and the last are the end states), ``chains`` chains
    each, ``equil`` steps and then one recorded (u_A, U_B) pair of every chain
    each ``stride`` steps until there are ``nsamples`` per state.  State 0 starts
    from ``prior.sample(chains)`` (or ``x0``), every later state from where the
    one before it ended; state k runs with ``seed + k``.  The pairs give
    ``u[n, k] = (1 - lam_k) u_A + lam_k U_B / kT`` of every sample in every state
    (in fp64, less each sample's minimum over the states, which MBAR does not see),
    ``mbar.mbar_solve`` gives f, and the result is ``((f_K - f_1) / nparticles *
    kT, its asymptotic error from mbar.mbar_std)`` as 0-d fp64 tensors.  The error
    treats the samples as independent: choose ``stride`` past the correlation
    time."""
    d = cfg.dataset
    lams = [float(v) for v in lambdas]
    if not 2 <= len(lams) <= 8:
        raise ValueError("fe_stratified takes 2 <= K <= 8 values of lambda, got %d" % len(lams))
    sw = _switch_for(cfg, prior, potential)
    nsamples, equil, stride = int(nsamples), int(equil), int(stride)
    if nsamples < 1 or equil < 0 or stride < 1:
        raise ValueError("fe_stratified needs nsamples >= 1, equil >= 0 and stride >= 1")
    chains = max(1, min(int(chains), nsamples))
    per = -(-nsamples // chains)
    x = prior.sample(chains) if x0 is None else x0
    x = _sim_positions(potential, x.detach().reshape(len(x), -1), d.dim)
    pairs = []
    for k, lam_k in enumerate(lams):
        lam = torch.full((equil + per * stride + 1,), lam_k)
        kw = dict(dt=dt, gamma=gamma, seed=int(seed) + k)
        sw.set_velocity(None)
        sw.switch(lam, nsteps=equil, init_pos=x, **kw)
        out = sw.switch(lam, nsteps=per * stride, record_every=stride, step0=equil, **kw)
        x = out[0]
        pairs.append(out[4].reshape(-1, 2)[:nsamples].double())
    en = torch.cat(pairs)  # the states' blocks in order
    lam_t = torch.tensor(lams, dtype=torch.float64, device=en.device)
    u = (1.0 - lam_t) * en[:, :1] + lam_t * (en[:, 1:] / d.kT)
    u = u - u.amin(dim=1, keepdim=True)
    if u.is_cuda:
        u = u.float()
    n_k = [nsamples] * len(lams)
    f, _, gram = mbar_.mbar_solve(u, n_k)
    K = len(lams)
    return ((f[0, K - 1] - f[0, 0]) / d.nparticles * d.kT,
            mbar_.mbar_std(gram, n_k, 0, K - 1)[0] / d.nparticles * d.kT)


def fe_diff_no_training(cfg, model, potential, nsamples):
    """test.py:74-88: the free energies of the model's prior (state 0) and the
    target (state 1) from ``nsamples`` samples of each, without the flow:
    ``kT * f / nparticles`` as a [2] fp64 tensor on the prior's device, f from
    ``mbar.mbar_solve`` in the gauge f_0 = 0 (the reference prints FastMBAR's
    ``F``).  Two deliberate differences from the reference's text: it scores
    ``traj0`` twice (line 79 evaluates the prior on the prior's own samples
    again, where the target's samples ``traj1`` are meant), and it divides by a
    literal 54; here the prior scores ``traj1`` and the divisor is
    ``cfg.dataset.nparticles``.  Nothing is plotted or printed."""
    d = cfg.dataset
    traj0 = model.prior.sample((nsamples,))
    q00 = model.prior.log_prob(traj0)
    q01 = -(potential.potential(traj0.reshape(-1, d.nparticles, d.dim)) / d.kT).detach().to(q00.device)
    traj1 = potential.sample(nsamples)
    traj1 = traj1.reshape(len(traj1), -1).to(q00.device)
    q10 = model.prior.log_prob(traj1)
    q11 = -(potential.potential(traj1.reshape(-1, d.nparticles, d.dim)) / d.kT).detach().to(q00.device)
    Q0 = torch.transpose(torch.vstack((q00, q01)), 0, 1)
    Q1 = torch.transpose(torch.vstack((q10, q11)), 0, 1)
    u = -torch.cat((Q0, Q1), dim=0).detach()
    f, _, _ = mbar_.mbar_solve(u, [len(traj0), len(traj1)])
    return d.kT * f[0] / d.nparticles
