"""Loader for the golden fixtures written by oracle/gen_golden.py (plain named arrays)."""
import glob
import os

import numpy as np
import torch

from oracle import rnb_oracle as O
from tests.parity import GRAD_CAP, K_GRAD

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# Calibrated gradient bounds are parity.grad_bound(rel32s), capped at GRAD_CAP (tests/parity.py).  A tensor whose
# fp32 REFERENCE gradient is further than GRAD_CAP / K_GRAD from the reference's fp64 gradient is something fp32 cannot
# resolve: it is not a parity target and must be listed here explicitly (fixture -> tensor names), otherwise the
# fixture refuses to load.  No committed fixture needs an entry (largest rel32s: 2.6e-3, tiny_warmup_sharp
# dev.variance).
UNRESOLVED_BY_FP32 = {}

# tests/golden/image_rays_small.npz: largest element difference between `interpolate_pose` and the reference's recorded pose
# over the fixture's three ratios, measured on the CPU: 0.0 (bit-equal: same float32 inversions, and the float64 slerp rounds
# to the same float32 rotation).  The bound is four times that and may not exceed 1e-5 (tests/test_image_render_host.py).
POSE_DIFF_MEASURED = 0.0
POSE_BOUND = 4.0 * POSE_DIFF_MEASURED


def case_names():
    """Renderer fixtures (tiny_* / full_*); raygen_* fixtures have their own loader below."""
    names = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))
    return [n for n in names if n.startswith("tiny_") or n.startswith("full_")]


def load_raygen(name="raygen_small"):
    """Golden vectors of the reference's per-step ray generation (oracle/gen_golden.py::raygen_case):
    returns (dataset tensors, list of cases)."""
    import torch
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
    ds = {k: torch.from_numpy(z[k]) for k in ("images", "images_warmup", "masks", "light_directions",
                                               "light_directions_warmup", "intrinsics_all_inv", "pose_all")}
    cases = []
    i = 0
    while f"c{i}_data" in z.files:
        pre = f"c{i}_"
        cases.append({k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)})
        i += 1
    return ds, cases


class Golden:
    def __init__(self, name):
        self.name = name
        z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
        self.z = z
        s = z["conf.sdf"]
        sf = z["conf.sdf_f"]
        c = z["conf.color"]
        r = z["conf.render"]
        rf = z["conf.render_f"]
        self.mc = O.ModelConf(
            sdf=O.SDFConf(d_in=int(s[0]), d_out=int(s[1]), d_hidden=int(s[2]), n_layers=int(s[3]),
                          skip_in=(int(s[4]),) if s[4] >= 0 else (), multires=int(s[5]),
                          bias=float(sf[0]), scale=float(sf[1])),
            color=O.ColorConf(d_feature=int(c[0]), d_in=int(c[1]), d_out=int(c[2]), d_hidden=int(c[3]),
                              n_layers=int(c[4]), multires_view=int(c[5])),
            render=O.RenderConf(n_samples=int(r[0]), n_importance=int(r[1]), n_outside=int(r[2]),
                                up_sample_steps=int(r[3]), perturb=float(rf[0])),
            init_val=float(rf[1]))
        self.api = str(z["meta.api"])
        self.cos_anneal_ratio = float(z["meta.cos_anneal_ratio"])
        self.no_albedo = bool(int(z["meta.no_albedo"]))
        self.perturb_overwrite = float(z["meta.perturb_overwrite"])
        self.grad_stride = int(z["meta.grad_stride"])
        self.batch = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in.")}
        self.out = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("out.")}
        self.grads = {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("grad.")}
        self.gradnorm = {k[9:]: float(z[k]) for k in z.files if k.startswith("gradnorm.")}
        self.n_steps = int(z["trace.n_steps"])
        self.steps = []
        for i in range(self.n_steps):
            pre = f"trace.{i}."
            self.steps.append({k[len(pre):]: torch.from_numpy(np.asarray(z[k])) for k in z.files
                               if k.startswith(pre)})
        # the sample positions the fine pass received (== steps[-1]["z_out"] when there is an up-sampling loop)
        self.z_fine = torch.from_numpy(z["trace.z_vals"])
        # the reference in fp64 on the same samples, and the fp32 reference's distance from it (gen_golden.py)
        self.out64 = {k[6:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("out64.")}
        self.grad64 = {k[7:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("grad64.")}
        self.grad64_stride = {k[14:]: int(z[k]) for k in z.files if k.startswith("grad64_stride.")}
        self.rel32 = {k[6:]: float(z[k]) for k in z.files if k.startswith("rel32.")}
        self.rel32s = {k[7:]: float(z[k]) for k in z.files if k.startswith("rel32s.")}
        dropped = set(UNRESOLVED_BY_FP32.get(name, ()))
        for k, r in self.rel32s.items():
            if r > GRAD_CAP / K_GRAD and k not in dropped:
                raise ValueError(f"fixture {name}: the fp32 reference's own gradient of {k} is {r:.2e} (rel-L2) from "
                                 f"its fp64 run — beyond GRAD_CAP / K_GRAD = {GRAD_CAP / K_GRAD:.1e}; list it in "
                                 "UNRESOLVED_BY_FP32 to drop it explicitly")
        for k in dropped:
            self.grad64.pop(k, None)
        self.weights_from = str(z["meta.weights_from"]) if "meta.weights_from" in z.files else None
        self.has_weights = any(k.startswith("w.") for k in z.files) or self.weights_from is not None
        self.wsum = {k[5:]: z[k] for k in z.files if k.startswith("wsum.")}

    def params(self, requires_grad=False):
        """Named parameters: stored arrays, or (full_*_geo) regenerated from seed 0 and verified
        against the stored checksums."""
        if self.weights_from is not None:     # same network state as another fixture (stored once)
            zw = np.load(os.path.join(GOLDEN_DIR, self.weights_from + ".npz"), allow_pickle=False)
            p = {k[2:]: torch.from_numpy(zw[k]).clone() for k in zw.files if k.startswith("w.")}
        elif self.has_weights:
            p = {k[2:]: torch.from_numpy(self.z[k]).clone() for k in self.z.files if k.startswith("w.")}
        else:
            torch.manual_seed(0)
            p = O.init_params(self.mc)
            for k, chk in self.wsum.items():
                d = p[k].double().reshape(-1)
                got = np.array([float(d.sum()), float((d * d).sum()), float(d[0]), float(d[-1])])
                np.testing.assert_allclose(got, chk, rtol=1e-12, atol=1e-12, err_msg=k)
        if requires_grad:
            for v in p.values():
                v.requires_grad_(True)
        return p

    def background_rgb(self):
        return self.batch.get("background_rgb")
