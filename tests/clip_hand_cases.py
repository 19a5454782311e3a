"""Gradient clipping worked by hand in numbers float32 holds exactly (3-4-5 triangles; scales that are dyadic fractions), so that every
expected value below is the real-number result and no rounding enters: what tests/np_clip.py must say, and what the device must do.

A case is one optimizer step over ONE two-element tensor: gradient `g`, weight `w`, `weight_decay`, the settings, and what must come
out: q (the sum of squares), norm, scale, whether the step counts as clipped / skipped, and `out`, the gradient the update rule receives
(None on a skipped step).  NaN in an expectation means "a NaN"."""
import numpy as np

nan, inf = float("nan"), float("inf")


def _case(name, g, out, q, norm, scale, clipped, w=(0.0, 0.0), weight_decay=0.0, clipnorm=None, clipvalue=None, skip_nonfinite=False,
          skipped=False):
    return dict(name=name, g=np.array(g, dtype=np.float32), w=np.array(w, dtype=np.float32), weight_decay=weight_decay,
                clipnorm=clipnorm, clipvalue=clipvalue, skip_nonfinite=skip_nonfinite,
                out=None if out is None else np.array(out, dtype=np.float32), q=q, norm=norm, scale=scale, clipped=clipped, skipped=skipped)


CASES = [
    # norm 5 against clipnorm 2.5: scale 1/2
    _case("halved", (3, 4), (1.5, 2), 25.0, 5.0, 0.5, True, clipnorm=2.5),
    # the boundary: norm >= clipnorm holds with equality, the scale is exactly 1 and the step counts as clipped
    _case("boundary", (3, 4), (3, 4), 25.0, 5.0, 1.0, True, clipnorm=5.0),
    # below the bound: untouched
    _case("below", (3, 4), (3, 4), 25.0, 5.0, 1.0, False, clipnorm=6.0),
    # the gradient alone has norm 3 < 3.75 ...
    _case("no_decay_no_clip", (3, 0), (3, 0), 9.0, 3.0, 1.0, False, w=(0, 8), clipnorm=3.75),
    # ... with the penalty's share 0.5 * (0, 8) it is (3, 4): norm 5 >= 3.75, scale 3/4
    _case("decay_makes_it_clip", (3, 0), (2.25, 3), 25.0, 5.0, 0.75, True, w=(0, 8), weight_decay=0.5, clipnorm=3.75),
    # clipvalue after clipnorm: (3, -4) -> (1.5, -2) -> (1.5, -1.75); clipvalue alone would have given (1.75, -1.75)
    _case("value_after_norm", (3, -4), (1.5, -1.75), 25.0, 5.0, 0.5, True, clipnorm=2.5, clipvalue=1.75),
    _case("value_alone", (3, -4), (1.75, -1.75), 25.0, 5.0, 1.0, False, clipvalue=1.75),
    # a NaN gradient: the norm is NaN, the comparison false, nothing is scaled; the clamp leaves the NaN a NaN
    _case("nan_row", (3, nan), (2, nan), nan, nan, 1.0, False, clipnorm=2.5, clipvalue=2.0),
    # an infinite gradient: norm inf, scale 2.5 / inf = 0, inf * 0 = NaN
    _case("inf_row", (3, inf), (0, nan), inf, inf, 0.0, True, clipnorm=2.5),
    # skip_nonfinite: the same two rows do nothing at all
    _case("nan_row_skipped", (3, nan), None, nan, nan, 1.0, False, clipnorm=2.5, skip_nonfinite=True, skipped=True),
    _case("inf_row_skipped", (3, inf), None, inf, inf, 0.0, False, clipnorm=2.5, skip_nonfinite=True, skipped=True),
    # skip_nonfinite alone: a finite step is the unclipped step
    _case("skip_option_finite", (3, 4), (3, 4), 25.0, 5.0, 1.0, False, skip_nonfinite=True),
]


def same(a, b):
    """Equal as float32 values, a NaN matching any NaN."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))
