"""MI355X-native drop-in for the MVS patch-expansion stage of
MarvinChung/simple-implementation-of-structure-from-motion-and-multi-view-stereo-by-python.

Import with importlib (the directory name is not an identifier):
    mvs = importlib.import_module(
        "simple-implementation-of-structure-from-motion-and-multi-view-stereo-by-python_amd")
"""
from . import _lib, sfm, synthetic, utils  # noqa: F401
from ._lib import MvsContext, ncc_windows, rodrigues_roundtrip, triangulate  # noqa: F401
from .MVS2 import (DensePointsWarped, DensePointsWithMVS2, MyPatch, densify_depth_warped, depth_maps_warped, expand_patches_warped,  # noqa: F401
                   filter_patches_warped, mesh_depth_warped, photo_consistency_batch, photo_consistency_warped, reconstruct_patches_warped,
                   refine_patches_warped, resume_patches_warped)
from .utils import (SeedSet, export2ply, export2ply_mesh, export2ply_oriented, read_imgs, read_pars, read_ply,  # noqa: F401
                    read_ply_mesh, read_ply_oriented)

PACKAGE = __name__
