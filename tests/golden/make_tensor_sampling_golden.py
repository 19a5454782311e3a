#!/usr/bin/env python3
"""Generate tensor_sampling.npz / tensor_sampling.json FROM THE REAL REFERENCE (misc_utils/tensor_sampling_utils.py).

    SSD_REFERENCE=<checkout of pierluigiferrari/ssd_keras> python tests/golden/make_tensor_sampling_golden.py

Like make_golden.py it imports the live reference at generation time and only then.  Every case seeds the global `np.random` stream,
calls the reference's `sample_tensors` and records: the inputs, the call's arguments, the outputs with their dtypes (or the exception's
type), and a digest of the `np.random` state the call left behind -- for the error cases too, since some errors come after draws.
The json also carries the `ast`-read signature of the reference's function (tests/api_surface.py).
tests/test_tensor_sampling_cpu.py pins ssd_keras_amd.misc_utils.tensor_sampling_utils to these files.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import api_surface  # noqa: E402

SURFACE = {"misc_utils/tensor_sampling_utils.py": ["sample_tensors"]}


def state_digest():
    """sha256 over the Mersenne Twister's key, its position and the cached second Gaussian of the legacy `normal`."""
    name, key, pos, has_gauss, cached = np.random.get_state()
    return hashlib.sha256(key.tobytes() + repr((name, int(pos), int(has_gauss), float(cached))).encode()).hexdigest()


def encode(inst):
    """JSON form of sampling instructions; what JSON cannot say is tagged: {"numpy_integer": 6}, {"tuple": [...]}."""
    if isinstance(inst, np.integer):
        return {"numpy_integer": int(inst)}
    if isinstance(inst, tuple):
        return {"tuple": [encode(i) for i in inst]}
    if isinstance(inst, list):
        return [encode(i) for i in inst]
    return inst


def cases():
    """(name, seed for the inputs, shapes, dtype, instructions, axes, init, mean, stddev)"""
    kb = [(3, 3, 4, 12), (12,)]
    f32, f64 = "float32", "float64"
    tutorial = [c + i * 4 for i in range(3) for c in (0, 2)]                     # 3 boxes x 4 classes -> 3 x 2
    out = [
        ("list_last_axis", kb, f32, [3, 3, 4, tutorial], [[3]], None, 0.0, 0.005),
        ("list_last_axis_f64", kb, f64, [3, 3, 4, tutorial], [[3]], None, 0.0, 0.005),
        ("list_last_axis_tuple", kb, f32, (3, 3, 4, tuple(tutorial)), [[3]], None, 0.0, 0.005),
        ("list_two_axes", [(3, 3, 4, 12), (4, 12)], f32, [3, 3, [3, 1], [0, 5, 11, 5]], [[2, 3]], None, 0.0, 0.005),
        ("list_negative_indices", kb, f32, [3, 3, 4, [0, -1, -12, 3]], [[3]], None, 0.0, 0.005),
        ("int_subsample", kb, f32, [3, 3, 4, 5], [[3]], None, 0.0, 0.005),
        ("int_subsample_f64", kb, f64, [3, 3, 4, 5], [[3]], None, 0.0, 0.005),
        ("int_subsample_two_axes", kb, f32, [3, 2, 4, 7], [[3]], None, 0.0, 0.005),
        ("int_subsample_to_one", kb, f32, [3, 3, 4, 1], [[3]], None, 0.0, 0.005),
        ("int_equal", kb, f32, [3, 3, 4, 12], [[3]], None, 0.0, 0.005),
        ("int_equal_unknown_init_unused", kb, f32, [3, 3, 4, 12], [[3]], ["ones", "ones"], 0.0, 0.005),
        ("upsample_init_none", kb, f32, [3, 3, 4, 18], [[3]], None, 0.0, 0.005),
        ("upsample_init_none_f64", kb, f64, [3, 3, 4, 18], [[3]], None, 0.0, 0.005),
        ("upsample_gaussian", kb, f32, [3, 3, 4, 18], [[3]], ["gaussian", "gaussian"], 0.25, 0.5),
        ("upsample_zeros", kb, f32, [3, 3, 4, 18], [[3]], ["zeros", "zeros"], 0.0, 0.005),
        ("upsample_gaussian_zeros", kb, f32, [3, 3, 4, 18], [[3]], ["gaussian", "zeros"], 0.0, 0.005),
        ("upsample_zeros_gaussian", kb, f64, [3, 3, 4, 18], [[3]], ["zeros", "gaussian"], 0.0, 0.005),
        ("upsample_two_axes", [(3, 3, 4, 12), (4, 12)], f32, [3, 3, 6, 15], [[2, 3]], None, 0.0, 0.005),
        ("subsample_one_upsample_other", [(3, 3, 4, 12), (4, 12)], f32, [3, 3, 2, 15], [[2, 3]], None, 0.0, 0.005),
        ("list_one_upsample_other", [(3, 3, 4, 12), (4, 12)], f32, [3, 3, 7, [0, 4, 8]], [[2, 3]], ["gaussian", "zeros"], 0.0, 0.005),
        ("three_tensors", [(3, 3, 4, 12), (12,), (4, 12)], f32, [3, 3, 3, 16], [[3], [2, 3]], None, 0.0, 0.005),
        ("three_tensors_lists", [(3, 3, 4, 12), (12,), (4, 12)], f64, [[2, 0], 3, [1, 2], tutorial], [[3], [2, 3]], None, 0.0, 0.005),
        ("single_tensor_axes_none_sub", [(5, 7)], f32, [3, [6, 0]], None, None, 0.0, 0.005),
        ("single_tensor_axes_none_up", [(5, 7)], f64, [8, 7], None, None, 1.0, 0.1),
        # the refusals
        ("error_instructions_too_short", kb, f32, [3, 3, 4], [[3]], None, 0.0, 0.005),
        ("error_instructions_too_long", kb, f32, [3, 3, 4, 12, 1], [[3]], None, 0.0, 0.005),
        ("error_init_too_short", kb, f32, [3, 3, 4, 18], [[3]], ["gaussian"], 0.0, 0.005),
        ("error_init_too_long_no_upsampling", kb, f32, [3, 3, 4, 12], [[3]], ["zeros"] * 3, 0.0, 0.005),
        ("error_index_equals_length", kb, f32, [3, 3, 4, [0, 12]], [[3]], None, 0.0, 0.005),
        ("error_index_beyond_length", kb, f32, [3, 3, [0, 9], [0, 1]], [[3]], None, 0.0, 0.005),
        ("error_numpy_integer", kb, f32, [3, 3, 4, np.int64(6)], [[3]], None, 0.0, 0.005),
        ("error_float_instruction", kb, f32, [3, 3, 4, 6.0], [[3]], None, 0.0, 0.005),
        ("error_unknown_init_first", kb, f32, [3, 3, 4, 18], [[3]], ["ones", "zeros"], 0.0, 0.005),
        ("error_unknown_init_second_after_draws", kb, f32, [3, 3, 4, 18], [[3]], ["gaussian", "ones"], 0.0, 0.005),
        ("error_after_subsampling_draw", kb, f32, [3, 3, 2, np.int64(6)], [[3]], None, 0.0, 0.005),
    ]
    return out


def main():
    ref = os.environ.get("SSD_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
    if not ref or not os.path.isdir(ref):
        sys.exit("set SSD_REFERENCE (or pass the path) to a checkout of the reference")
    sys.path.insert(0, ref)
    from misc_utils.tensor_sampling_utils import sample_tensors
    arrays, manifest = {}, {"signature": api_surface.extract(ref, SURFACE), "cases": {}}
    for n, (name, shapes, dtype, inst, axes, init, mean, stddev) in enumerate(cases()):
        seed = 1000 + n
        rng = np.random.RandomState(seed)
        inputs = [rng.standard_normal(s).astype(dtype) for s in shapes]
        for i, a in enumerate(inputs):
            arrays["%s/in/%d" % (name, i)] = a
        entry = {"seed": seed, "n_inputs": len(inputs), "instructions": encode(inst), "axes": axes, "init": init, "mean": mean, "stddev": stddev}
        np.random.seed(seed)
        try:
            outs = sample_tensors([a.copy() for a in inputs], inst, axes=axes, init=init, mean=mean, stddev=stddev)
        except Exception as e:                                           # noqa: BLE001 -- the type is what is recorded
            if not name.startswith("error_"):
                raise
            entry["error"] = type(e).__name__
        else:
            assert not name.startswith("error_"), name
            entry["out_dtypes"] = [str(o.dtype) for o in outs]
            entry["out_shapes"] = [list(o.shape) for o in outs]
            for i, o in enumerate(outs):
                arrays["%s/out/%d" % (name, i)] = o
        entry["state"] = state_digest()
        manifest["cases"][name] = entry
    np.savez_compressed(os.path.join(HERE, "tensor_sampling.npz"), **arrays)
    with open(os.path.join(HERE, "tensor_sampling.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
    print("%d cases, %d arrays" % (len(manifest["cases"]), len(arrays)))


if __name__ == "__main__":
    main()
