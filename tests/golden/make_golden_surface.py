"""Generate tests/golden/surface.npz from the REFERENCE's own evaluation/SurfaceDice.py.

    MLAGG_REFERENCE=<reference checkout> python tests/golden/make_golden_surface.py

Stores, for tests/_surface_cases.py:
  - area/<i>: the per-code surfel areas at AREA_SPACINGS[i], by the loop at the top of compute_surface_distances (:322-334) over the
    reference's neighbour_code_to_normals;
  - mask/<case>/<key>: compute_surface_distances' four lists, and the four metrics on them (compute_surface_dice_at_tolerance and
    compute_surface_overlap_at_tolerance at TOLERANCES, compute_average_surface_distance, compute_robust_hausdorff at PERCENTS);
  - label/<case>/nsd and nsd_rounded: the per-organ loop of the *_NSD_Eval.py scripts (:90-110), restated because they read NIfTI
    files through argparse.
numpy 2 has no np.Inf, which the reference uses for an empty surface: it is set to np.inf first.  Only the data is committed."""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if "MLAGG_REFERENCE" not in os.environ:
    raise SystemExit("set MLAGG_REFERENCE to a checkout of the reference repository (aticejiang/MLAgg-UNet)")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(os.environ["MLAGG_REFERENCE"], "evaluation"))
np.Inf = np.inf

import SurfaceDice as S  # noqa: E402

import mlagg_unet_amd  # noqa: E402,F401
from tests import _surface_cases as C  # noqa: E402


def reference_areas(spacing_mm):
    out = np.zeros(256)
    for code in range(256):
        normals = np.array(S.neighbour_code_to_normals[code])
        sum_area = 0
        for k in range(normals.shape[0]):
            n = np.zeros([3])
            n[0] = normals[k, 0] * spacing_mm[1] * spacing_mm[2]
            n[1] = normals[k, 1] * spacing_mm[0] * spacing_mm[2]
            n[2] = normals[k, 2] * spacing_mm[0] * spacing_mm[1]
            sum_area += np.linalg.norm(n)
        out[code] = sum_area
    return out


def find_lower_upper_zbound(organ_mask):
    z_index = np.where(np.uint8(organ_mask) > 0)[2]
    return np.min(z_index), np.max(z_index)


def script_nsd(gt_data, seg_data, spacing, tolerances, slab_labels):
    out = []
    for i, organ in enumerate(tolerances.keys(), 1):
        if np.sum(gt_data == i) == 0 and np.sum(seg_data == i) == 0:
            nsd = 1
        elif np.sum(gt_data == i) == 0 and np.sum(seg_data == i) > 0:
            nsd = 0
        else:
            if i in slab_labels:
                z_lower, z_upper = find_lower_upper_zbound(gt_data == i)
                g, s = gt_data[:, :, z_lower:z_upper] == i, seg_data[:, :, z_lower:z_upper] == i
            else:
                g, s = gt_data == i, seg_data == i
            nsd = S.compute_surface_dice_at_tolerance(S.compute_surface_distances(g, s, spacing), tolerances[organ])
        out.append(nsd)
    return np.array(out, np.float64), np.array([round(v, 4) for v in out], np.float64)


def main():
    warnings.simplefilter("ignore", RuntimeWarning)          # 0 / 0 of empty surfaces, as in the scripts
    g = {"area_spacings": np.array([[float(v) for v in s] for s in C.AREA_SPACINGS])}
    for i, s in enumerate(C.AREA_SPACINGS):
        g[f"area/{i}"] = reference_areas(s)
    for name, mg, mp, sp in C.mask_cases():
        sd = S.compute_surface_distances(mg, mp, sp)
        for k, v in sd.items():
            g[f"mask/{name}/{k}"] = np.asarray(v, np.float64)
        g[f"mask/{name}/dice"] = np.array([S.compute_surface_dice_at_tolerance(sd, t) for t in C.TOLERANCES])
        g[f"mask/{name}/overlap"] = np.array([S.compute_surface_overlap_at_tolerance(sd, t) for t in C.TOLERANCES])
        g[f"mask/{name}/average"] = np.array(S.compute_average_surface_distance(sd))
        g[f"mask/{name}/hausdorff"] = np.array([S.compute_robust_hausdorff(sd, p) for p in C.PERCENTS], np.float64)
    for name, gt, seg, sp, tol, slabs in C.label_cases():
        g[f"label/{name}/nsd"], g[f"label/{name}/nsd_rounded"] = script_nsd(gt, seg, sp, tol, slabs)
    path = C.golden_path()
    np.savez_compressed(path, **g)
    print(f"wrote {path}: {len(g)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
