"""sitator_amd: the landmark-analysis hot path of sitator, MI355X-native.

Host code is Python and talks to hand-written HIP kernels (gfx950) through the ctypes C-ABI of
``include/sitator_hip.h``.  The public names mirror the reference package for this path::

    from sitator_amd import SiteNetwork, SiteTrajectory, LandmarkAnalysis
    st = LandmarkAnalysis(clustering_algorithm="dotprod").run(sn, frames)
"""
from .errors import (CoordinationEnvironmentError, InsufficientSitesError, LandmarkAnalysisError, MultipleOccupancyError,  # noqa: F401
                     StaticLatticeError, VoronoiError, ZeroLandmarkError)
from .site_network import SiteNetwork, Structure  # noqa: F401
from .site_trajectory import SiteGrouping, SiteTrajectory  # noqa: F401
from .pbc import PBCCalculator  # noqa: F401
from .dotprod_classifier import DotProdClassifier, LandmarkVectors  # noqa: F401
from .landmark import LandmarkAnalysis  # noqa: F401
from .dynamics import (AverageVibrationalFrequency, GenerateClampedTrajectory, JumpAnalysis, MergeSitesByDynamics,  # noqa: F401
                       MergeSitesByThreshold, RemoveUnoccupiedSites, ReplaceUnassignedPositions, SmoothSiteTrajectory)
from .dynamics import MeanSquaredDisplacement, MSDResult, diffusion_coefficient  # noqa: F401
from .dynamics import VanHoveCorrelation, VanHoveResult, RadialDistribution, RDFResult  # noqa: F401
from .dynamics import IntermediateScattering, ScatteringResult, StructureFactor, StructureFactorResult, q_vectors  # noqa: F401
from .density import DensityResult, IonicDensity, gaussian_stencil  # noqa: F401
from .percolation import ComponentsResult, PercolationResult, density_components, density_percolation  # noqa: F401
from .landscape import EnergyLandscape, LandscapeResult  # noqa: F401
from .merging import MergeSites, MergeSitesError, MergedSitesTooDistantError  # noqa: F401
from .recenter import RecenterTrajectory  # noqa: F401
from .misc import GenerateAroundSites, NAvgsPerSite  # noqa: F401
from .network import DiffusionPathwayAnalysis, MergeSitesByBarrier  # noqa: F401
from .voronoi import VoronoiSiteGenerator  # noqa: F401
from . import calculators  # noqa: F401
from .site_descriptors import (InsufficientCoordinatingAtomsError, SiteCoordinationEnvironment, SiteTypeAnalysis, SiteVolumes, SOAP,  # noqa: F401
                               SOAPCenters, SOAPDescriptorAverages, SOAPSampledCenters, device_soap_backend)
from .descriptors import ConfigurationalEntropy  # noqa: F401

__version__ = "0.1.0"
