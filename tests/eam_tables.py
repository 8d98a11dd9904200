"""Synthetic single-element setfl tables for the EAM tests (a helper, not a
test module).  Two families:

* ``cubic``: F, f and z = r phi are cubic polynomials and rc sits on the last
  r node, so the interpolant of systems.EAM is exact away from the first and
  last two intervals and the energy has a closed form.
* ``fs``: Finnis-Sinclair-shaped functions, F = -A sqrt(rho),
  f = (r - d)^2 + b (r - d)^3 / d below d and z = r (r - c)^2 (c0 + c1 r +
  c2 r^2) below c (both zero beyond), rc = max(c, d).  The parameters are test
  inputs only; nothing rides on their being anyone's iron.
"""
import numpy as np

# polynomial coefficients, lowest power first
CUBIC_F = (0.0, -1.3, 0.21, -0.011)      # F(rho)
CUBIC_f = (2.0, -1.1, 0.35, -0.06)       # f(r)
CUBIC_z = (3.0, -2.2, 0.9, -0.17)        # z(r) = r phi(r)


def poly(c, x):
    return ((c[3] * x + c[2]) * x + c[1]) * x + c[0]


def dpoly(c, x):
    return (3 * c[3] * x + 2 * c[2]) * x + c[1]


def cubic(rc=2.0, nr=201, nrho=201, rho_max=40.0):
    """Cubic-polynomial tables with rc on the last r node."""
    dr, drho = rc / (nr - 1), rho_max / (nrho - 1)
    r, rho = dr * np.arange(nr), drho * np.arange(nrho)
    return dict(element="Xx", element_line=["26", "55.845", "2.8553", "bcc"], nrho=nrho, drho=drho, nr=nr,
                dr=dr, rc=rc, F=poly(CUBIC_F, rho), f=poly(CUBIC_f, r), z=poly(CUBIC_z, r))


def fs(scale=1.0, nr=2000, nrho=2000, rho_max=60.0, A=1.9, d=3.7, b=-0.9, c=3.4, c0=1.2, c1=-0.6, c2=0.09):
    """Finnis-Sinclair-shaped tables; ``scale`` stretches every length (d, c
    and with them rc)."""
    d, c = d * scale, c * scale
    rc = max(c, d)
    dr, drho = rc / (nr - 1), rho_max / (nrho - 1)
    r, rho = dr * np.arange(nr), drho * np.arange(nrho)
    f = np.where(r < d, (r - d) ** 2 + b * (r - d) ** 3 / d, 0.0)
    z = np.where(r < c, r * (r - c) ** 2 * (c0 + c1 * r + c2 * r * r), 0.0)
    return dict(element="Xx", element_line=["26", "55.845", "2.8553", "bcc"], nrho=nrho, drho=drho, nr=nr,
                dr=dr, rc=rc, F=-A * np.sqrt(rho), f=f, z=z)


def write_setfl(path, tab, per_line=5):
    """Write ``tab`` as a setfl file with ``per_line`` values per line."""
    vals = np.concatenate((tab["F"], tab["f"], tab["z"]))
    with open(path, "w") as fh:
        fh.write("synthetic table\nfor the EAM tests\nno physical meaning\n")
        fh.write("1 %s\n" % tab["element"])
        fh.write("%d %.17g %d %.17g %.17g\n" % (tab["nrho"], tab["drho"], tab["nr"], tab["dr"], tab["rc"]))
        fh.write(" ".join(tab["element_line"]) + "\n")
        for i in range(0, len(vals), per_line):
            fh.write(" ".join("%.17g" % v for v in vals[i:i + per_line]) + "\n")
    return str(path)


def bcc(ncell, a, jitter=0.0, seed=0, batch=None):
    """A bcc lattice of ncell^3 cells (2 ncell^3 atoms) with lattice constant
    a, optionally perturbed: [n, 3], or [batch, n, 3] of independent
    perturbations (fp64)."""
    g = np.arange(ncell)
    corner = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    pos = np.concatenate((corner, corner + 0.5)) * a
    rng = np.random.default_rng(seed)
    if batch is None:
        return pos + jitter * rng.standard_normal(pos.shape)
    return pos + jitter * rng.standard_normal((batch,) + pos.shape)


FE_YAML = """
device : cpu
dataset :
  name : Fe_test
  potential : Fe
  training_data : %(data)s
  testing_data : %(data)s
  input_dir : ../data/fe/in.lmp
  %(eam)s
  nparticles : 16
  kT : 0.00861733326
  ncellx : 2
  ncelly : 2
  ncellz : 2
  cell_len : 2.8841
flow:
  type: NSF_AR
  nlayers: 1
  nsplines: 8
  hidden_dim: 32
prior:
  type : EinsteinCrystal
  centers : %(centers)s
  alpha : 600
"""


def fe_config(tmp_path, with_eam=True, device="cpu"):
    """An Fe-style config (16 atoms, bcc 2x2x2, EinsteinCrystal prior, 1-layer
    NSF_AR) with its setfl table and 12 training frames written into tmp_path:
    (cfg, table, frames)."""
    a = 2.8841
    tab = fs(scale=0.95)
    eam_path = write_setfl(tmp_path / "Xx.eam.fs", tab)
    # centred on the origin: the flow's splines act on [-B, B], B = ncellx * cell_len / 2
    frames = (bcc(2, a, jitter=0.03, seed=9, batch=12) - 0.75 * a).astype(np.float32)
    np.save(tmp_path / "train.npy", frames)
    centers = (bcc(2, a) - 0.75 * a).round(6).tolist()
    text = FE_YAML % dict(data=str(tmp_path / "train.npy"), centers=centers,
                          eam="eam_file : %s" % eam_path if with_eam else "sigma : 1.0")
    p = tmp_path / "fe.yaml"
    p.write_text(text.replace("device : cpu", "device : %s" % device))
    from normalizingflow_amd import app
    return app.read_input(str(p)), tab, frames
