"""gftorf_amd -- MI355X-native differentiable ToF Gaussian rasterizer.

Drop-in for the reference's ``diff_gaussian_rasterization_w_tof`` extension
(brownvc/gftorf, submodules/diff-gaussian-rasterization-w-tof): same Python
operator API, hand-written gfx950 HIP kernels behind a C ABI
(include/gftorf_rast.h).  See DESIGN.md.
"""
from . import reproducible  # noqa: F401  (first: api, flow and deform read the switch; the module is callable)
from .reproducible import set_reproducible, is_reproducible  # noqa: F401
from .api import (GaussianRasterizationSettings, GaussianRasterizer, rasterize_gaussians,  # noqa: F401
                  _RasterizeGaussians)
from .pair import GaussianRasterizerPair, render_pair  # noqa: F401
from .assemble import assemble_inputs, assemble_parameters  # noqa: F401
from .knn import distCUDA2  # noqa: F401
from .optim import FusedAdam, clip_grad_norm_  # noqa: F401
from .deform import DeformNetwork, REFERENCE_ARCH, reference_network  # noqa: F401
from . import densify  # noqa: F401
from . import loss  # noqa: F401
from . import flow  # noqa: F401
from . import reg  # noqa: F401
from . import rigid  # noqa: F401
from . import tof  # noqa: F401
from . import query  # noqa: F401
from . import metrics  # noqa: F401
from . import present  # noqa: F401
from . import tracks  # noqa: F401
from . import ply  # noqa: F401
from . import pcd  # noqa: F401
from . import png  # noqa: F401
from . import views  # noqa: F401
from . import schedule  # noqa: F401
from .query import DeformQuery, ftorf_schedule, query_dmlp  # noqa: F401
from .views import DrawOrder, ViewStore, select_plane  # noqa: F401
from .schedule import RunSchedule  # noqa: F401
from .rigid import Neighbours, find_knn, isometry_loss, rigid_terms, rigidity_loss  # noqa: F401

__all__ = ["GaussianRasterizationSettings", "GaussianRasterizer", "rasterize_gaussians", "GaussianRasterizerPair", "render_pair", "assemble_inputs", "assemble_parameters", "distCUDA2", "FusedAdam", "clip_grad_norm_",
           "DeformNetwork", "REFERENCE_ARCH", "reference_network", "densify",
           "DeformQuery", "ftorf_schedule", "query_dmlp", "views", "ViewStore", "DrawOrder", "select_plane", "schedule", "RunSchedule",
           "reproducible", "set_reproducible", "is_reproducible",
           "rigid", "Neighbours", "find_knn", "rigidity_loss", "isometry_loss", "rigid_terms"]
