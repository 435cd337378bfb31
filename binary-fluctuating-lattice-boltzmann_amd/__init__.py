"""MI355X-native D3Q19 binary fluctuating-LBM collide-and-stream path.

Import name: the directory name contains hyphens, so load it through
``__graft_entry__.load_package()`` (registers it as ``bflbm_amd``) or importlib.
The product path needs the HIP library csrc/libbflbm.so; there is no CPU fallback.
"""
from . import _lib
from ._lib import BflbmError, Params, Domain, Fab, NVEL, NHYDRO, NHYDROBAR, HALO_STATE, HALO_NEXT, HALO_UPLOAD
from .lattice import BinaryLBM, RingLBM, BatchLBM, Trace, InterfaceTrace, ShapeTrace, SpectrumTrace, ModeTrace, FieldStats, ProfileTrace, HistogramTrace, MorphologyTrace, ChordTrace, CoarseTrace, LagTrace, MomentTrace, ClusterTrace, ComponentTrace, RadialTrace, default_params, make_fab, rng_site_normals, fused_plan_query, sweep_plan_query
from .slab import SlabLattice, LocalSlabRing, slab_bounds
from . import plotfile
from . import analysis
from . import structfact
from .structfact import BatchStructFact
from . import run_job

__all__ = ["RingLBM", "BatchLBM", "Trace", "InterfaceTrace", "ShapeTrace", "SpectrumTrace", "ModeTrace", "FieldStats", "ProfileTrace", "HistogramTrace", "MorphologyTrace", "ChordTrace", "CoarseTrace", "LagTrace", "MomentTrace", "ClusterTrace", "ComponentTrace", "RadialTrace", "BatchStructFact", "SlabLattice", "LocalSlabRing", "slab_bounds", "BinaryLBM", "default_params", "make_fab", "rng_site_normals", "fused_plan_query", "sweep_plan_query", "BflbmError",
           "Params", "Domain", "Fab", "NVEL", "NHYDRO", "NHYDROBAR"]
