"""CPU: the float partial-sum knots of the fused NSF epilogue are no less
accurate than the 2^-30 fixed-point prefixes they replace (fp32 emulation of
both forms against the float64 reference formula, tools/knot_forms.py), and
their edges stay strictly increasing."""
import importlib.util
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("knot_forms", os.path.join(REPO, "tools", "knot_forms.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("sigma", [0.3, 1.0, 3.0])
def test_float_knots_no_worse_than_fixed_point(sigma):
    err, mono = _tool().knot_errors(sigma, sets=100000, seed=int(10 * sigma))
    print("sigma %.1f: max / p99 / mean fixed %.3g / %.3g / %.3g, float %.3g / %.3g / %.3g"
          % ((sigma,) + err["fixed"] + err["float"]))
    assert mono["float"] and mono["fixed"]
    assert err["float"][0] <= 1.1 * err["fixed"][0]
    assert err["float"][1] <= 1.1 * err["fixed"][1]
    # both sit at the fp32 rounding of a knot in [-3, 3] (ulp 2.4e-7), not above a few of them
    assert err["float"][0] < 4e-6
