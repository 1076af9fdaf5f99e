"""What a Renderer keeps of the objects it creates for frame images (vulkan_renderer_amd/frame_images.py): one registry for
the statistics, the filters and the histories, which Renderer.close() walks."""
import pytest

from vulkan_renderer_amd import renderer

pytestmark = pytest.mark.gpu


def test_closing_the_renderer_destroys_every_frame_object():
    """A renderer with nothing but its device - none of the three needs a scene or a pass - and one object of each kind"""
    r = renderer.Renderer()
    try:
        frame_filter, history, statistics = r.create_frame_filter(16, 16), r.create_frame_history(16, 16), r.create_statistics(256)
        assert frame_filter.filter.filtered and (frame_filter.width, frame_filter.height) == (16, 16)
        assert history.history.accumulated and (history.width, history.height) == (16, 16)
        assert statistics.stats.sums and statistics.pixel_count == 256
    finally:
        r.close()
    assert not frame_filter.filter.filtered and frame_filter.filter.width == 0
    assert not history.history.accumulated and history.history.width == 0
    assert not statistics.stats.sums and statistics.stats.pixel_count == 0
    # closing what the renderer closed does nothing
    for frame_object in (frame_filter, history, statistics):
        frame_object.close()
    assert not frame_filter.filter.filtered and not history.history.accumulated and not statistics.stats.sums
