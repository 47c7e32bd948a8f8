"""isochrones_amd — MI355X-native implementation of the isochrones hot path
(DFInterpolator N-D interpolation -> interp_mag -> star_lnlike -> StarModel.lnpost).

Host side: Python mirroring the reference's interface for this path; compute: hand-written
HIP kernels for gfx950 behind the C ABI in include/isochrones_amd.h (no CPU fallback)."""
from .interp import DFInterpolator
from .models import (ModelGridInterpolator, EvolutionTrackInterpolator, IsochroneInterpolator,
                     synthetic_track, synthetic_isochrone, get_ichrone)
from .starmodel import (BasicStarModel, StarModel, TreeStarModel, SingleStarModel, BinaryStarModel,
                        TripleStarModel, IsoTrackModel)
from .observation import ObservationTree, Observation, Source
from ._cabi import IsoError
from .sampler import EnsembleSampler, FusedEnsembleSampler
from .catalog import (StarCatalog, CatalogPosterior, fit_catalog, synthetic_catalog, shard_of, shard_indices,
                      broadcast_interpolator, fit_stars_nested_gpu, nested_result_columns, nested_max_live,
                      select_multiplicity)
from . import priors, grids, ingest, mist, nested, ini, persist, utils
from .starfit import starfit, batch_starfit
from .cluster import StarClusterModel, combine_star_moments, simulate_cluster
from .diagnostics import chain_diagnostics, ChainDiagnostics
from .derived import chain_derived
from .predictive import chain_predictive
from . import populations
from .populations import (StarPopulation, BinaryDistribution, StarFormationHistory, StarFormationHistoryGrid, deredden,
                          evaluate_binaries)
from . import hierarchical
from .hierarchical import PopulationModel, PopulationPosterior, PowerLaw, TruncatedGaussian, Fixed
from . import reweight
from . import selection
from .selection import InjectionSet
from . import relations
from .relations import LinearGaussian
from . import binned
from .binned import Histogram
from . import draws
from .draws import DrawPlan
from . import binfit
from .binfit import BinnedFit
from . import emfit
from .emfit import BinnedBootstrap

__version__ = "0.1.0"
