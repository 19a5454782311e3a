#!/usr/bin/env python3
"""Generate tests/golden/data_generator/ (fixture images, a CSV and a COCO-style JSON file), data_generator.npz and
api_surface_data_generator.json FROM THE REAL REFERENCE.

Run where a checkout of the reference exists (SSD_REFERENCE = its root; default: a sibling directory named `reference`):

    python tests/golden/make_data_generator_golden.py

It runs the reference's DataGenerator (data_generator/object_detection_2d_data_generator.py) unmodified: its parsers on the fixture files
and three batches of `generate()` each for `[SSDDataAugmentation(300, 300)]` (shuffled, crossing an epoch wrap) and `[ConvertTo3Channels,
Resize(300, 300)]` (with inverters and the original labels), recording the `np.random` state behind every batch.  OpenCV is not
installed: the modules run with the `cv2` of make_golden.py (oracle/np_image.py's restatement of cvtColor / resize); h5py and
BeautifulSoup are not needed for these calls.  Needs sklearn, PIL and tqdm."""
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
import sklearn.utils  # noqa: E402,F401  (before the aliases below: SciPy's numpy.ma import breaks on them)
np.float = float   # noqa: aliases removed in NumPy >= 1.24, used by the reference
np.int = int       # noqa
np.bool = bool     # noqa

from tests import api_surface                 # noqa: E402
from tests import data_generator_cases as dc  # noqa: E402

SURFACE = {"data_generator/object_detection_2d_data_generator.py": [
    "DataGenerator.__init__", "DataGenerator.load_hdf5_dataset", "DataGenerator.parse_csv", "DataGenerator.parse_xml",
    "DataGenerator.parse_json", "DataGenerator.create_hdf5_dataset", "DataGenerator.generate", "DataGenerator.save_dataset",
    "DataGenerator.get_dataset", "DataGenerator.get_dataset_size"]}


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
    return cv2


def main():
    dc.write_fixtures()
    for name in [m for m in sys.modules if m == "cv2" or m.startswith(("data_generator", "ssd_encoder_decoder", "bounding_box_utils"))]:
        del sys.modules[name]
    sys.modules["cv2"] = stub_cv2()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")              # the reference warns that h5py / bs4 are missing
        import data_generator.object_detection_2d_data_generator as odg
    from data_generator.data_augmentation_chain_original_ssd import SSDDataAugmentation
    from data_generator.object_detection_2d_geometric_ops import Resize
    from data_generator.object_detection_2d_photometric_ops import ConvertTo3Channels
    ns = types.SimpleNamespace(DataGenerator=odg.DataGenerator, SSDDataAugmentation=SSDDataAugmentation, Resize=Resize,
                               ConvertTo3Channels=ConvertTo3Channels)
    out = dc.run_reference(ns)
    path = os.path.join(HERE, "data_generator.npz")
    np.savez_compressed(path, **out)
    print("%-28s %8.1f KB  %d arrays" % ("data_generator", os.path.getsize(path) / 1024.0, len(out)))
    surface = api_surface.extract(REF, surface=SURFACE)
    missing = [(m, q) for m, d in surface.items() for q, v in d.items() if v is None]
    assert not missing, missing
    with open(os.path.join(HERE, "api_surface_data_generator.json"), "w") as f:
        json.dump(surface, f, indent=0, sort_keys=True)


if __name__ == "__main__":
    main()
