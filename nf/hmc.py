"""nf.hmc: the reference's module name for normalizingflow_amd.hmc."""
from normalizingflow_amd.hmc import *  # noqa: F401,F403
from normalizingflow_amd.hmc import HMC  # noqa: F401
