"""--dump-outputs DIR: what the timed path computed in its last step, as DIR/<name>.npy, so that two builds of the project can
be compared output for output (the inputs of a run are seeded: the same arguments give the same inputs)."""
import ctypes
import os

import numpy as np

OUTPUT_LIMIT_BYTES = 64 << 20
SAMPLE_SEED = 20240613


def timed_outputs(r, exchange, slab):
    """The frame a caller of the timed step receives, read right after the timed region: the radiance target (one rank, or the
    frame every rank holds after the all-gather of rgba32f slabs), the encoded RGB8 frame when that is what was exchanged, or
    the rank's slab when slabs stay where they are (--exchange none).  float32 arrays by name."""
    if exchange == "rgb8":
        e = r.app.swapchain.extent
        encoded = np.zeros((e.height, e.width, 4), np.uint8)
        if r.lib.read_back_encoded(ctypes.byref(r.app), encoded.ctypes.data):
            raise RuntimeError("read_back_encoded failed")
        return {"encoded": encoded.astype(np.float32)}
    if slab is not None:
        r.finish_frames()
        r.sync()
        return {"slab": slab.cpu().numpy().astype(np.float32)}
    return {"radiance": r.read_radiance()}


def write_outputs(directory, arrays, limit=OUTPUT_LIMIT_BYTES):
    """Writes every array as <directory>/<name>.npy.  If they hold more than `limit` bytes together, each is cut to a fixed,
    seeded sample of its pixels (rows over the last axis, in ascending order) and the sampled pixel indices are written beside
    it as <name>_pixel_index.npy (float64); the sample depends only on the array's shape.  Returns the names written."""
    os.makedirs(directory, exist_ok=True)
    total = sum(a.nbytes for a in arrays.values())
    written = []
    for name, array in arrays.items():
        array = np.ascontiguousarray(array)
        assert array.dtype in (np.float32, np.float64), (name, array.dtype)
        if total > limit:
            pixels = array.reshape(-1, array.shape[-1])
            # (the sample and its index share the array's part of the limit)
            count = min(len(pixels), int(limit * array.nbytes / total) // (pixels.itemsize * pixels.shape[1] + 8))
            index = np.sort(np.random.default_rng(SAMPLE_SEED).choice(len(pixels), size=count, replace=False))
            np.save(os.path.join(directory, name + "_pixel_index.npy"), index.astype(np.float64))
            written.append(name + "_pixel_index")
            array = pixels[index]
        np.save(os.path.join(directory, name + ".npy"), array)
        written.append(name)
    return written
