"""Golden fixture for the elastic distortion (run where the reference is readable; the fixture is committed, the
reference is not read at test time).  Loads the reference's own `dataset/dataset_utils/data_processing.py` by
path (it imports numpy and scipy) and records, for two cases (scale 50 and scale 20) of ~2,000 points in a
centred box of 5 x 4 x 2.6 m times scale:

  * the points (f64) and gran / mag of both fields (`dataset/data.py:172-173`);
  * the output of `elastic(x, 6*scale//50, 40*scale/50)` and of `elastic(., 20*scale//50, 160*scale/50)` applied
    to it, in sequence from one seeded np.random stream (f64);
  * per field bb and the raw noise (f32): np.random is reseeded and `randn(*bb)` x 3 redrawn per field, which is
    the stream the reference consumed;
  * per field the three blurred grids (f32) as the reference hands them to its interpolator (recorded by
    wrapping `scipy.interpolate.RegularGridInterpolator` while the reference runs).

It asserts that every output coordinate is more than 1e-6 from an integer, so a test that truncates the
coordinates cannot flip on an evaluation-order difference.

    python tests/golden/make_elastic_golden.py <path to the reference checkout>
"""
import importlib.util
import os
import sys
import warnings

import numpy as np
import scipy.interpolate

if len(sys.argv) != 2:
    raise SystemExit(__doc__)
ref_root = sys.argv[1]

spec = importlib.util.spec_from_file_location(
    "ref_data_processing", os.path.join(ref_root, "dataset", "dataset_utils", "data_processing.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

captured = []
_RGI = scipy.interpolate.RegularGridInterpolator


def recording_rgi(axes, values, *args, **kwargs):
    captured.append(np.array(values, copy=True))
    return _RGI(axes, values, *args, **kwargs)


SEED = {50: 11, 20: 12}
out = {"scales": np.asarray([50, 20], np.int64)}
for scale in (50, 20):
    rng = np.random.RandomState(100 + scale)
    x = (rng.rand(2000, 3) - 0.5) * np.array([5.0, 4.0, 2.6]) * scale
    fields = [(6 * scale // 50, 40 * scale / 50), (20 * scale // 50, 160 * scale / 50)]
    np.random.seed(SEED[scale])
    captured.clear()
    scipy.interpolate.RegularGridInterpolator = recording_rgi
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)  # the scipy.ndimage.filters namespace
            y1 = ref.elastic(x, *fields[0])
            y2 = ref.elastic(y1, *fields[1])
    finally:
        scipy.interpolate.RegularGridInterpolator = _RGI
    assert len(captured) == 6
    np.random.seed(SEED[scale])
    for f, (xin, (gran, mag)) in enumerate(zip((x, y1), fields), 1):
        bb = np.abs(xin).max(0).astype(np.int32) // gran + 3
        raw = np.stack([np.random.randn(bb[0], bb[1], bb[2]).astype("float32") for _ in range(3)])
        blurred = np.stack(captured[3 * (f - 1):3 * f])
        assert blurred.shape == raw.shape and blurred.dtype == np.float32
        out[f"bb{f}_{scale}"], out[f"raw{f}_{scale}"], out[f"blur{f}_{scale}"] = bb.astype(np.int64), raw, blurred
        out[f"gran{f}_{scale}"], out[f"mag{f}_{scale}"] = np.int64(gran), np.float64(mag)
    for y in (y1, y2):
        clear = np.abs(y - np.round(y)).min()
        assert clear > 1e-6, f"scale {scale}: a coordinate lies {clear} from an integer; pick another seed"
    out[f"x_{scale}"], out[f"y1_{scale}"], out[f"y2_{scale}"] = x, y1, y2
    print(f"scale {scale}: bb1 {out[f'bb1_{scale}']} bb2 {out[f'bb2_{scale}']} max|y1-x| {np.abs(y1 - x).max():.3f} "
          f"max|y2-y1| {np.abs(y2 - y1).max():.3f}")

here = os.path.dirname(os.path.abspath(__file__))
path = os.path.join(here, "elastic_field.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
