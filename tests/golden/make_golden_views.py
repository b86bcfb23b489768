"""tests/golden/make_golden_views.py -- the view poses of the reference's textured-keypoint tool, produced by RUNNING THE REFERENCE
(build container only; needs the reference tree, oracle/ref_harness.REF_ROOT):  python tests/golden/make_golden_views.py

The reference's utils/dataset_tools/utils.py is loaded with its third-party imports stubbed (cv2, scipy, plyfile: PoseUtils uses
none of them), the way make_golden_train.py loads the datasets; nothing in the reference is edited.  For every case the lines of
rgbd_rnder_sift_kp3ds.py:142-156 are followed with the reference's own PoseUtils:
    sph_r = r / 0.035 * 0.18;  CameraPositions(n1, n2, sph_r);  getCameraPose;  get_o2c_pose_cv(cam_pose, np.eye(4))
Stored in view_poses.npz (a few KB): radius f64 [C], n1 i64 [C], n2 i64 [C], and poses{c} f64 [V,4,4] per case.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

CASES = [(0.035, 3, 3), (0.11, 3, 3), (0.035, 2, 4), (0.11, 2, 4)]


def reference_pose_utils():
    from oracle.ref_harness import REF_FFB6D
    for name in ("cv2", "scipy", "scipy.stats", "plyfile"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["scipy"].stats = sys.modules["scipy.stats"]
    sys.modules["plyfile"].PlyData = None
    spec = importlib.util.spec_from_file_location("ffb6d_reference_dataset_tools_utils",
                                                  os.path.join(REF_FFB6D, "utils", "dataset_tools", "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.PoseUtils()


def main():
    pose_utils = reference_pose_utils()
    out = dict(radius=np.array([c[0] for c in CASES]), n1=np.array([c[1] for c in CASES]), n2=np.array([c[2] for c in CASES]))
    for c, (r, n1, n2) in enumerate(CASES):
        sph_r = r / 0.035 * 0.18
        positions = pose_utils.CameraPositions(n1, n2, sph_r)
        cam_poses = [pose_utils.getCameraPose(pos) for pos in positions]
        out[f"poses{c}"] = np.array([pose_utils.get_o2c_pose_cv(cam_pose, np.eye(4)) for cam_pose in cam_poses])
    path = os.path.join(HERE, "view_poses.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
