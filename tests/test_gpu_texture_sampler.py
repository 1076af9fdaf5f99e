"""The device's material texture sampler (sample_texture() of csrc/shading_inputs.h) on its own, through
evaluate_device_texture_sampler: every tap count at every level of textures that are square or not, powers of two or not, with
whole or truncated chains, at coordinates from texel centres to NaN.  In the libm and the exact arithmetic mode the device must
equal the CPU oracle bit for bit; the fast mode is held to the binary64 restatement of tests/sampler_cases.py.  That the inputs
cover what they claim to - from the restatement's count, never from the device's output - is asserted here and in
tests/test_textures.py (no GPU needed).  Then one rendered frame per mode, which adds the
loader, the upload and the descriptor packing of resolve_material()."""
import functools

import numpy as np
import pytest

import golden_cases
import oracle
import sampler_cases
from helpers import compare, oracle_render
from test_gpu_parity import RMSE_TOLERANCE
from vulkan_renderer_amd import renderer, synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    r = renderer.Renderer()
    yield r
    r.close()


@functools.lru_cache(maxsize=None)
def oracle_samples(name, srgb, math_mode):
    oracle.set_math_mode(math_mode)
    try:
        return oracle.sample_texture_batch(dict(sampler_cases.make_texture(name), srgb=srgb), sampler_cases.make_inputs(name))
    finally:
        oracle.set_math_mode(0)


@pytest.mark.parametrize("arithmetic", ["libm", "exact"])
@pytest.mark.parametrize("srgb", [0, 1], ids=["linear", "srgb"])
@pytest.mark.parametrize("name", sampler_cases.TEXTURE_IDS)
def test_device_sampler_equals_the_oracle_in_every_bit(device, name, srgb, arithmetic):
    texture, inputs = dict(sampler_cases.make_texture(name), srgb=srgb), sampler_cases.make_inputs(name)
    sampler_cases.assert_coverage(name)
    got = device.sample_texture(texture, inputs, arithmetic)
    want = oracle_samples(name, srgb, renderer.ORACLE_MATH_MODE[arithmetic])
    same = sampler_cases.same_bits(got, want)
    assert same.all(), (int((~same).sum()), inputs[~same][:4], got[~same][:4], want[~same][:4])
    # NaN only where a coordinate or a derivative is not finite
    assert not np.isnan(got[np.isfinite(inputs).all(axis=1)]).any()


@pytest.mark.parametrize("name", sampler_cases.TEXTURE_IDS)
def test_fast_device_sampler_stays_near_the_restatement(device, name):
    """v_rcp_f32, v_sqrt_f32, v_log_f32 and contraction instead of IEEE operations: no bit-exact partner, so the fast kernel is
    held to the binary64 restatement.  Inputs whose tap count changes when P_max / P_min or P_max move by 1e-3 of themselves
    are left out - a discontinuity of the function, not an error; the inputs keep away from these steps, at most 1 % are.  The
    bound is measured, not chosen: the largest absolute difference of the exact-mode ORACLE from the restatement on the same
    inputs, times 8 (v_rcp_f32's 1 ulp and contraction over at most 16 taps).  It is taken twice: as it is - which the coordinates
    of 10^6 and more decide, where float32 has no fraction of a texel left and the difference is a whole texel for both - and in
    units of sampler_cases.tolerance(), 2^-21 (4 + |u| w + |v| h), which weighs every input by what float32 can resolve there.

    Measured on an MI355X (profiles/r15_summary.md has every texture):
    oracle (exact mode) against the restatement, then the fast kernel, largest over linear and sRGB:
      1x1             3.3e-8   6.0e-8    in units of the tolerance  0.017  0.031
      5x3             0.82     0.82                                 0.10   0.11
      48x20, 3 levels 0.82     0.82                                 0.20   0.29
      8x8, 2 levels   0.91     0.91                                 0.26   0.43
      256x16          0.67     0.67                                 0.094  0.12
      32x32           0.69     0.69                                 0.15   0.14
    (the absolute figures of all but 1x1 belong to coordinates of 10^6 and more, where both read the same wrong texel)"""
    inputs = sampler_cases.make_inputs(name)
    want, footprint = sampler_cases.restated(name)
    kept = ~footprint["tap_steps"]
    print(name, "on a step of the tap count: %.3f %% of the inputs" % (100.0 * (~kept).mean()))
    assert (~kept).mean() <= 0.01
    scale = sampler_cases.tolerance(sampler_cases.make_texture(name), inputs)[:, None]
    for srgb in (0, 1):
        got = device.sample_texture(dict(sampler_cases.make_texture(name), srgb=srgb), inputs, "fast").astype(np.float64)
        exact = oracle_samples(name, srgb, 1).astype(np.float64)
        assert not np.isnan(got[kept & ~np.isnan(exact).any(axis=1)]).any()
        rows = kept & np.isfinite(want[:, srgb]).all(axis=1) & np.isfinite(exact).all(axis=1)
        oracle_error, fast_error = np.abs(exact - want[:, srgb])[rows], np.abs(got - want[:, srgb])[rows]
        figures = (oracle_error.max(), fast_error.max(), (oracle_error / scale[rows]).max(), (fast_error / scale[rows]).max())
        print(name, "srgb", srgb, "largest difference from the restatement: oracle (exact mode) %.3e, fast kernel %.3e; in units of the float32 tolerance: %.4f, %.4f" % figures)
        assert figures[1] <= 8.0 * figures[0], figures
        assert figures[3] <= 8.0 * figures[2], figures


# ---- frames ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def grazing_dataset(tmp_path_factory):
    return synthetic.write_dataset(str(tmp_path_factory.mktemp("grazing")), **sampler_cases.GRAZING_DATASET)


@pytest.mark.parametrize("arithmetic", ["libm", "exact", "fast"])
def test_grazing_textured_frame_equals_the_oracle(arithmetic, grazing_dataset):
    """Textures of 96x40 with five of their seven levels under a camera that grazes the ground plane: the frame reaches level 3
    and 16 taps (asserted), through the loader, the upload and the descriptors that the sampler tests above bypass"""
    r = renderer.Renderer(arithmetic=arithmetic)
    sampler_cases.apply_grazing_case(r, golden_cases.TEXTURED_CASES[2], grazing_dataset)
    r.create_targets()
    r.create_pass()
    r.render_visibility()
    r.render()
    image = r.read_radiance()
    cpu, inputs, bvh = oracle_render(r, visibility=r.read_visibility(), math_mode=renderer.ORACLE_MATH_MODE[arithmetic])
    sampler_cases.assert_frame_works_the_sampler(oracle.make_frame(inputs, r.oracle_settings(), bvh), inputs["material_textures"])
    r.close()
    stats = compare(image, cpu)
    print(arithmetic, stats)
    if arithmetic == "fast":
        assert stats["nan"] == 0 and stats["rmse"] <= RMSE_TOLERANCE, stats
    else:
        assert stats["bit_exact"], stats
