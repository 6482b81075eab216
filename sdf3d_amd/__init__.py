"""sdf3d_amd -- MI355X-native SDF sphere-tracing renderer.

Drop-in replacement for the device programs of ezorzin/SDF3D
(Code/shader/voxel_fragment.frag et al.): a hand-written HIP kernel for
gfx950 behind the C-ABI in include/sdf_abi.h.  This package holds the ctypes
binding (abi), the scene/camera presets (scenes), the host-side renderer
(renderer), what sdf_measure's rows mean (measure), OBJ mesh files (meshio),
the torch.autograd layer over sdf_sample_grad (autograd, imported on demand: it
needs torch), the multi-device frame driver (multigpu) and the algorithmic cost
model used for roofline accounting (costmodel).
"""
from . import abi, scenes
from .abi import SdfError, load_library
from .measure import Measure, fit_grid
from .renderer import Grad, Mesh, Renderer, owned_rows, tiling
from .scenes import CONFIGS, Frame, config, orbit_view, reference

__all__ = ["abi", "scenes", "SdfError", "load_library", "Grad", "Measure", "Mesh", "Renderer",
           "fit_grid", "owned_rows", "tiling", "CONFIGS", "Frame", "config", "orbit_view",
           "reference"]
