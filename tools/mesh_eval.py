"""Distance between two meshes on the device: accuracy, completeness, Chamfer, sampled Hausdorff, precision / recall /
F-score (`rnb_neus_fork_amd.mesh_distance`; point-to-triangle distances, exact for the samples drawn).

  python tools/mesh_eval.py A.ply B.ply [--samples N] [--threshold TAU ...] [--seed S] [--error-ply OUT.ply [--error-max D]]

A is the mesh under test, B the reference, both as `write_ply` writes them and in the same coordinates (no alignment is
done).  Prints ONE JSON line.  `--error-ply` writes the samples drawn on A as a point cloud coloured by their distance to B
(blue 0 .. red `--error-max`, default the largest distance)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def error_colors(distance, d_max):
    """[n,3] floats in [0, 1]: blue at 0 through green to red at d_max"""
    x = np.clip(np.asarray(distance, dtype=np.float64) / d_max, 0.0, 1.0) if d_max > 0 else np.zeros(len(distance))
    return np.stack([np.clip(2.0 * x - 1.0, 0.0, 1.0), 1.0 - np.abs(2.0 * x - 1.0), np.clip(1.0 - 2.0 * x, 0.0, 1.0)], axis=1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mesh_a")
    ap.add_argument("mesh_b")
    ap.add_argument("--samples", type=int, default=1_000_000, help="samples per surface")
    ap.add_argument("--threshold", type=float, action="append", default=[], help="F-score threshold (repeatable)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--error-ply", help="write the samples of A coloured by their distance to B here")
    ap.add_argument("--error-max", type=float, help="distance shown as red (default: the largest)")
    a = ap.parse_args(argv)
    sys.path.insert(0, ROOT)
    import rnb_neus_fork_amd as R

    if not torch.cuda.is_available():
        raise SystemExit("tools/mesh_eval.py needs a GPU (there is no CPU path)")
    dev = torch.device("cuda:0")
    meshes = []
    for path in (a.mesh_a, a.mesh_b):
        m = R.read_ply(path)
        meshes += [torch.from_numpy(np.ascontiguousarray(m["vertices"], dtype=np.float64)).to(dev),
                   torch.from_numpy(np.ascontiguousarray(m["triangles"], dtype=np.int32)).to(dev)]
    out = R.mesh_distance(*meshes, n_samples=a.samples, thresholds=a.threshold, seed=a.seed,
                          return_samples=a.error_ply is not None)
    if a.error_ply:
        d = out.pop("distance_a").cpu().numpy()
        pts = out.pop("samples_a").cpu().numpy()
        out.pop("samples_b"), out.pop("distance_b")
        d_max = a.error_max if a.error_max is not None else float(d.max())
        R.write_ply(a.error_ply, pts, np.zeros((0, 3), dtype=np.int32), colors=error_colors(d, d_max))
        out["error_ply"] = {"path": a.error_ply, "points": len(pts), "red_at": d_max}
    out.update(mesh_a=a.mesh_a, mesh_b=a.mesh_b, vertices=(len(meshes[0]), len(meshes[2])), triangles=(len(meshes[1]), len(meshes[3])),
               seed=a.seed, build=R.native.build_id())
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
