#!/usr/bin/env python3
"""Generate tests/golden/affine_ops.npz and api_surface_affine.json FROM THE REAL REFERENCE.

Run where a checkout of the reference exists (SSD_REFERENCE = its root; default: a sibling directory named `reference`):

    python tests/golden/make_affine_golden.py

It runs the reference's Translate / Scale / Rotate and their random forms (data_generator/object_detection_2d_geometric_ops.py:233-772)
and its constant-input-size, variable-input-size and satellite chains unmodified on the seeded cases of tests/affine_cases.py.  OpenCV is
not installed: the modules run with a `cv2` built on oracle/np_image.py (cvtColor / resize) and tests/np_warp.py (getRotationMatrix2D,
warpAffine restated from imgwarp.cpp).  So these vectors pin everything the reference does AROUND those primitives -- random draws and
their generators, trial loops, label arithmetic, validation, filtering, clipping, dtypes -- and the primitives through their restatement."""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = os.environ.get("SSD_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
sys.path.insert(0, REF)
np.float = float   # noqa: aliases removed in NumPy >= 1.24, used by the reference
np.int = int       # noqa
np.bool = bool     # noqa

from tests import affine_cases as ac        # noqa: E402
from tests import api_surface               # noqa: E402
from tests import np_warp                   # noqa: E402

SURFACE = {
    "data_generator/object_detection_2d_geometric_ops.py": [q for c in ac.OPS for q in (c + ".__init__", c + ".__call__")],
    "data_generator/data_augmentation_chain_constant_input_size.py": ["DataAugmentationConstantInputSize.__init__",
                                                                      "DataAugmentationConstantInputSize.__call__"],
    "data_generator/data_augmentation_chain_variable_input_size.py": ["DataAugmentationVariableInputSize.__init__",
                                                                      "DataAugmentationVariableInputSize.__call__"],
    "data_generator/data_augmentation_chain_satellite.py": ["DataAugmentationSatellite.__init__", "DataAugmentationSatellite.__call__"],
}


def stub_cv2():
    from oracle import np_image as npi
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_RGB2HSV, cv2.COLOR_HSV2RGB, cv2.COLOR_RGB2GRAY = npi.COLOR_RGB2HSV, npi.COLOR_HSV2RGB, npi.COLOR_RGB2GRAY
    cv2.INTER_NEAREST, cv2.INTER_LINEAR, cv2.INTER_CUBIC, cv2.INTER_AREA, cv2.INTER_LANCZOS4 = 0, 1, 2, 3, 4
    cv2.BORDER_CONSTANT = 0
    cv2.cvtColor = lambda image, code: npi.cvt_color(np.ascontiguousarray(image), code)
    cv2.LUT = lambda image, table: npi.lut(image, table)
    cv2.equalizeHist = lambda plane: npi.equalize_hist(np.ascontiguousarray(plane))
    cv2.resize = lambda image, dsize=None, interpolation=1: npi.resize(np.ascontiguousarray(image), dsize, interpolation)
    cv2.getRotationMatrix2D = lambda center, angle, scale: np_warp.get_rotation_matrix_2d(center, angle, scale)

    def warp_affine(src, M, dsize, flags=1, borderMode=0, borderValue=0):
        assert flags == 1 and borderMode == 0, "only INTER_LINEAR / BORDER_CONSTANT are restated"
        return np_warp.warp_affine(np.ascontiguousarray(src), M, dsize, borderValue)
    cv2.warpAffine = warp_affine
    return cv2


def main():
    for name in [m for m in sys.modules if m == "cv2" or m.startswith("data_generator")]:
        del sys.modules[name]
    sys.modules["cv2"] = stub_cv2()
    import data_generator.object_detection_2d_geometric_ops as geo
    import data_generator.object_detection_2d_image_boxes_validation_utils as val
    import data_generator.data_augmentation_chain_constant_input_size as c1
    import data_generator.data_augmentation_chain_variable_input_size as c2
    import data_generator.data_augmentation_chain_satellite as c3
    ns = types.SimpleNamespace(BoxFilter=val.BoxFilter, ImageValidator=val.ImageValidator,
                               DataAugmentationConstantInputSize=c1.DataAugmentationConstantInputSize,
                               DataAugmentationVariableInputSize=c2.DataAugmentationVariableInputSize,
                               DataAugmentationSatellite=c3.DataAugmentationSatellite)
    for name in ac.OPS:
        setattr(ns, name, getattr(geo, name))
    out = {"n_cases": np.array(len(ac.CASES))}
    for i, case in enumerate(ac.CASES):
        for k, v in ac.run(ns, case).items():
            out["a%03d_%s" % (i, k)] = v
        out["a%03d_case" % i] = np.array(repr(case))
    path = os.path.join(HERE, "affine_ops.npz")
    np.savez_compressed(path, **out)
    print("%-28s %8.1f KB  %d arrays" % ("affine_ops", os.path.getsize(path) / 1024.0, len(out)))
    surface = api_surface.extract(REF, surface=SURFACE)
    missing = [(m, q) for m, d in surface.items() for q, v in d.items() if v is None]
    assert not missing, missing
    with open(os.path.join(HERE, "api_surface_affine.json"), "w") as f:
        json.dump(surface, f, indent=0, sort_keys=True)
    for name in [m for m in sys.modules if m == "cv2" or m.startswith("data_generator")]:
        del sys.modules[name]


if __name__ == "__main__":
    main()
