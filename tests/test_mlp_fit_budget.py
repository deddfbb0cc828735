"""Register budget of the MLP fit's kernels (csrc/mlp_fit.hip), from the compiler's resource remarks the build records:
the step and update kernels of a fit run thousands of times in a row and must not spill."""
import json

import pytest

from fdengine.build import RESOURCES


@pytest.fixture(scope="module")
def res():
    if not RESOURCES.exists():
        pytest.skip("no kernel_resources.json: build the library first (__graft_entry__.build())")
    return json.loads(RESOURCES.read_text())


@pytest.mark.parametrize("kernel", ["mlp_fit_step_kernel", "mlp_fit_update_kernel", "mlp_fit_mask_kernel"])
def test_mlp_fit_kernels_do_not_spill(res, kernel):
    hits = {k: v for k, v in res.items() if kernel in k}
    assert hits, f"no kernel matching {kernel}"
    for name, v in hits.items():
        assert v["scratch"] == 0, f"{name} spills {v['scratch']} B/lane"


def test_step_kernel_fits_several_waves_per_cu(res):
    """a workgroup is one wave with 36 KiB of LDS: at least four fit a CU's 160 KiB"""
    (v,) = [v for k, v in res.items() if "mlp_fit_step_kernel" in k]
    assert v["lds"] * 4 <= 160 * 1024 and v["vgpr"] + v["agpr"] <= 512
