"""normalizingflow_amd -- MI355X-native coupling-layer hot path of
sherryli59/NormalizingFlow (flows' forward/inverse + log|det J| on HIP kernels).

Public surface mirrors the reference (re-exported as the ``nf`` package):
    from nf.flows import RealNVP, NSF_CL, NSF_AR, Planar, Radial, FCNN
    from nf.models import NormalizingFlowModel   # also NormalizingFlow
    from nf.utils import unconstrained_RQS, RQS, searchsorted
The applications' priors and targets (applications/src/systems.py):
    from normalizingflow_amd.systems import EinsteinCrystal, GaussianMixture, LJ
Structure of a batch of configurations (no reference counterpart):
    from normalizingflow_amd.observables import pair_histogram, rdf, coordination
Counter-based random numbers of the device, restated for the CPU:
    from normalizingflow_amd.rng import philox4x32, philox_words, philox_normal
"""
from . import config  # noqa: F401
from . import systems  # noqa: F401
from ._lib import LIB_PATH, load as load_library  # noqa: F401
from .flows import FCNN, NSF_AR, NSF_CL, Planar, Radial, RealNVP  # noqa: F401
from .flows import MAF, ActNorm, OneByOneConv  # noqa: F401
from .flows import flush_status_checks  # noqa: F401
from .models import NormalizingFlow, NormalizingFlowModel  # noqa: F401

__version__ = "0.1.0"
