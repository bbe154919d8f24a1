"""Entry point with the reference's flags (main.py:33-42 of the reference):

    python main.py -img_p data/dinoRing -par_p data/dinoRing/dinoR_par.txt -t png -scale 10 \
                   -seeds tests/golden/seeds_dino.npz

The MVS stage (DensePointsWithMVS2, MVS2.py:176) runs on the GPU through
libmvs_amd.so and writes initial_patches.ply / all_patches.ply in the working
directory, like the reference.  Under torchrun (one process per GPU) the
expansion sweeps are sharded over the GPUs:

    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 main.py -img_p ... -seeds ...

Tracks: without -seeds, StructureFromMotion (SFM.py:47-88) runs first with the
reference's Harris/NCC features (HarrisFeatures.py) matched on the GPU in
place of OpenCV's ORB + FLANN + RANSAC (absent from this image); with -seeds
FILE.npz (track_off, obs_view, obs_xy, the format tests/golden/make_seeds.py
and -save_tracks write) the tracks are read instead.

--warped runs the warped pipeline instead (MVS2.DensePointsWarped: seeds from
Harris features along epipolar lines, expand -> filter) and writes
warped_patches.ply, an oriented point cloud; it needs neither SfM nor -seeds:

    python main.py -img_p data/dinoRing -par_p data/dinoRing/dinoR_par.txt -t png --warped

With -depth_maps DIR [-depth_radius R] it also renders per-view depth and normal
maps from the patches (DIR/depth_%04d.npy, DIR/normal_%04d.npy) and writes the
dense cloud fused from them as warped_dense.ply.  With -densify N on top of that
the maps are first densified by N sweeps of per-pixel plane propagation
(MvsContext.densify_depth's default schedule, at most 12): the densified maps are
written instead, with DIR/score_%04d.npy, and warped_dense.ply is fused from them.
With -mesh N the maps (densified when -densify is given) are also fused into a
signed-distance lattice of N voxels along its longest side and the surface is
written as warped_mesh.ply, a coloured triangle mesh (MvsContext.mesh_depth).
"""
import importlib
import os
import sys
from argparse import ArgumentParser

REPO = os.path.dirname(os.path.abspath(__file__))
PKG_NAME = "simple-implementation-of-structure-from-motion-and-multi-view-stereo-by-python_amd"
sys.path.insert(0, REPO)


def main(args, threshold=0.01, MIN_REPROJECTION_ERROR=0.3):
    mvs = importlib.import_module(PKG_NAME)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        # one process per GPU (torchrun): the expansion sweeps are sharded over
        # the ranks and exchanged with RCCL (parallel.stage_sharded)
        import torch
        import torch.distributed as dist
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        if not dist.is_initialized():
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    imgs = mvs.read_imgs(args)
    if getattr(args, "warped", False):
        # the warped pipeline in place of SfM and the stage: seeds from Harris
        # features along epipolar lines, expand -> filter, warped_patches.ply
        # with normals (MVS2.DensePointsWarped); single process
        mvs.DensePointsWarped(imgs, args, rounds=args.warped_rounds, iterations=args.warped_iterations,
                              epi_px=args.epi_px, expand={"cell_size": args.cell_size},
                              depth_maps=args.depth_maps, depth_radius=args.depth_radius, densify=getattr(args, "densify", 0),
                              mesh=getattr(args, "mesh", 0))
        return
    if getattr(args, "seeds", None):
        global_set = mvs.SeedSet.load(args.seeds)
    else:
        # SfM.StructureFromMotion (main.py:28) with the Harris/NCC front-end on
        # the GPU in place of OpenCV's ORB/FLANN/RANSAC (sfm.py)
        global_set = mvs.sfm.GlobalSet(threshold=threshold)
        st = mvs.sfm.StructureFromMotion(imgs, global_set, args, MIN_REPROJECTION_ERROR)
        n_obs, n_pts, _ = global_set.getInfo()
        print(f"SfM: {st['pairs']} pairs, {st['correspondences']} correspondences, "
              f"{st['kept']} triangulated, {n_pts} tracks / {n_obs} observations")
    if getattr(args, "save_tracks", None) and (world == 1 or int(os.environ.get("RANK", "0")) == 0):
        import numpy as np
        off, view, xy = mvs.utils.tracks_to_arrays(global_set.getInfo()[2])
        np.savez(args.save_tracks, track_off=off, obs_view=view, obs_xy=xy)
    mvs.DensePointsWithMVS2(imgs, global_set, args, max_pops=getattr(args, "max_pops", 100000))
    st = mvs.MVS2.last_stats
    if world == 1 or int(os.environ.get("RANK", "0")) == 0:
        print("pops {pops} tests {tests} accepted {accepts} gpu-scored {scored} sweeps {sweeps}".format(**st))


if __name__ == "__main__":
    parser = ArgumentParser()
    parser.add_argument("-img_p", help="image directory", dest="img_dir", default=None)
    parser.add_argument("-par_p", help="parameter path", dest="par_path", default=None)
    parser.add_argument("-t", help="image file type", dest="img_type", default="ppm")
    parser.add_argument("-scale", help="scale", dest="scale", default=1, type=float)
    parser.add_argument("--debug", help="debug mode on", dest="debug", action="store_true")
    parser.add_argument("--nonSequence", help="", dest="nonSeq", action="store_true")
    parser.add_argument("-cell_size", help="", dest="cell_size", default=2, type=int)
    parser.add_argument("-desc_wid", help="", dest="desc_wid", default=5, type=int)
    parser.add_argument("-seeds", help="SfM tracks (npz: track_off, obs_view, obs_xy)",
                        dest="seeds", default=None)
    parser.add_argument("-max_pops", help="expansion pop cap (<= 100000)", dest="max_pops",
                        default=100000, type=int)
    parser.add_argument("--filter_outliers", dest="filter_outliers", action="store_true",
                        help="run CellTable.filter_out_outlier before the reconstruction (the "
                             "reference has the call commented out, MVS2.py:281)")
    parser.add_argument("-save_tracks", help="write the SfM tracks (npz) before the MVS stage",
                        dest="save_tracks", default=None)
    parser.add_argument("--warped", dest="warped", action="store_true",
                        help="run the warped pipeline (feature seeds, expand, filter) in place of SfM and "
                             "the stage; writes warped_patches.ply with normals; needs no -seeds")
    parser.add_argument("-warped_rounds", dest="warped_rounds", default=4, type=int,
                        help="--warped: expansion rounds from the seeds")
    parser.add_argument("-warped_iterations", dest="warped_iterations", default=3, type=int,
                        help="--warped: filter / resumption iterations")
    parser.add_argument("-epi_px", dest="epi_px", default=1.5, type=float,
                        help="--warped: the seed matcher's distance from the epipolar line, pixels")
    parser.add_argument("-depth_maps", dest="depth_maps", default=None,
                        help="--warped: a directory for per-view depth_%%04d.npy and normal_%%04d.npy maps; the "
                             "cloud fused from them goes to warped_dense.ply")
    parser.add_argument("-depth_radius", dest="depth_radius", default=1, type=int,
                        help="--warped -depth_maps: the splat's footprint radius in pixels, 0..3")
    parser.add_argument("-densify", dest="densify", default=0, type=int,
                        help="--warped -depth_maps: densify the maps by this many sweeps of per-pixel plane "
                             "propagation (the default schedule: 1..12, anything above is refused; 0: none); needs -depth_maps")
    parser.add_argument("-mesh", dest="mesh", default=0, type=int,
                        help="--warped -depth_maps: fuse the maps into a signed-distance lattice of this many voxels "
                             "along its longest side and write the surface as warped_mesh.ply (0: none); needs "
                             "-depth_maps")
    args = parser.parse_args()
    if args.mesh < 0 or (args.mesh > 0 and not (args.warped and args.depth_maps)):
        parser.error("-mesh N needs N >= 0, --warped and -depth_maps DIR")
    try:
        main(args)
    except RuntimeError as e:
        print("RuntimeError", e)
        sys.exit(1)
