"""What a Renderer makes of whole frame images outside the pass: the objects behind create_statistics(),
create_frame_filter() and create_frame_history() (csrc/frame_images.h states what the last two share on the device), the
device memory that one call owns, and what the command lines of feature_buffers.py, frame_filter.py and frame_history.py
share.  renderer.py imports the classes: they are used under its name."""
import contextlib
import ctypes as C
import os

import numpy as np

from . import capi

_HIP_RUNTIME = None


def _hip_runtime():
    """The HIP runtime that the library has loaded, opened once, with the signatures of the three calls that the file
    encoders' encode_image() makes"""
    global _HIP_RUNTIME
    if _HIP_RUNTIME is None:
        hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes, hip.hipMalloc.restype = [C.POINTER(C.c_void_p), C.c_size_t], C.c_int
        hip.hipMemcpy.argtypes, hip.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
        hip.hipFree.argtypes, hip.hipFree.restype = [C.c_void_p], C.c_int
        _HIP_RUNTIME = hip
    return _HIP_RUNTIME


def _address(pointer):
    """An int, a ctypes pointer or None as an address"""
    return int(getattr(pointer, "value", pointer) or 0)


class _DeviceScratch:
    """Device memory that one call owns: `with _DeviceScratch(renderer, what) as scratch`.  On exit the renderer waits
    for the device if anything was allocated - a kernel may still use it - and all of it is freed.  `what` names the
    memory in the error messages ("an image of the filter"), `wrong_shape` begins the ValueError of upload()."""

    def __init__(self, owner, what, wrong_shape=None):
        self.owner, self.what, self.wrong_shape = owner, what, wrong_shape
        self.hip, self.owned = _hip_runtime(), []

    def __enter__(self):
        return self

    def allocate(self, nbytes, what=None):
        address = C.c_void_p()
        if self.hip.hipMalloc(C.byref(address), max(nbytes, 16)):
            raise RuntimeError("no device memory for %s" % (what or self.what))
        self.owned.append(address)
        return address.value

    def upload(self, array, shape=None, dtype=np.float32, what=None):
        """The address of a copy of the array, which is `shape` (None: any) of `dtype` (None: its own)"""
        array = np.ascontiguousarray(array, dtype)
        if shape is not None and array.shape != shape:
            raise ValueError("%s is %r, not %r" % (self.wrong_shape, shape, array.shape))
        address = self.allocate(array.nbytes)
        if self.hip.hipMemcpy(address, array.ctypes.data, array.nbytes, 1):
            raise RuntimeError("uploading %s failed" % (what or self.what))
        return address

    @staticmethod
    def download(address, shape, dtype, what):
        """Device memory as an array; the caller has waited for whoever writes it"""
        out = np.zeros(shape, dtype)
        if _hip_runtime().hipMemcpy(out.ctypes.data, address, out.nbytes, 2):
            raise RuntimeError("reading %s back failed" % what)
        return out

    def __exit__(self, *exception):
        if self.owned:
            self.owner.sync()
        for address in self.owned:
            self.hip.hipFree(address)
        return False


class _FrameObject:
    """An object of the C-ABI that a Renderer creates for frame images and closes with itself at the latest:
    `STRUCT` of capi, made by create_<NAME>() and released by destroy_<NAME>(), alive while its member `ALIVE` is set."""
    NAME = STRUCT = ALIVE = None

    def __init__(self, owner, *create_arguments):
        self.owner, self.lib = owner, owner.lib
        self.struct = self.STRUCT()
        if getattr(self.lib, "create_" + self.NAME)(C.byref(self.struct), C.byref(owner.app), *create_arguments):
            raise RuntimeError("create_%s failed" % self.NAME)
        owner._frame_objects.append(self)

    @property
    def alive(self):
        return bool(getattr(self.struct, self.ALIVE))

    def close(self):
        if self.alive:
            getattr(self.lib, "destroy_" + self.NAME)(C.byref(self.struct), C.byref(self.owner.app))
        if self in self.owner._frame_objects:
            self.owner._frame_objects.remove(self)


class FrameStatistics(_FrameObject):
    """Renderer.create_statistics(): sums of frames in binary64 on the device, mean and variance from them.  mean() and
    variance() return numpy arrays (pixels, 4); mean_into() / variance_into() write device buffers instead."""
    NAME, STRUCT, ALIVE = "frame_statistics", capi.FrameStatistics, "sums"

    def __init__(self, owner, pixel_count=None):
        super().__init__(owner, int(pixel_count or 0))
        self.stats = self.struct
        self._hip = C.CDLL("libamdhip64.so")
        self._scratch = C.c_void_p()

    @property
    def pixel_count(self):
        return int(self.stats.pixel_count)

    @property
    def frame_count(self):
        return int(self.stats.frame_count)

    def accumulate(self, pointers=None):
        """Adds the RGBA32F device buffers `pointers` (1 ... 8 addresses, in that order) with one kernel; None: the
        radiance target.  Returns at once."""
        if pointers is None:
            array, count = None, 1
        else:
            values = [_address(p) for p in pointers]
            array, count = (C.c_void_p * len(values))(*values), len(values)
        if self.lib.accumulate_frames(C.byref(self.stats), C.byref(self.owner.app), array, count):
            raise RuntimeError("accumulate_frames failed")

    def resolve(self, mean_pointer=None, variance_pointer=None):
        """Writes mean and / or variance into RGBA32F device buffers (resolve_frame_statistics)"""
        if self.lib.resolve_frame_statistics(C.byref(self.stats), C.byref(self.owner.app), mean_pointer, variance_pointer):
            raise RuntimeError("resolve_frame_statistics failed")

    def _resolved(self, want_variance):
        nbytes = 16 * self.pixel_count
        if not self._scratch and self._hip.hipMalloc(C.byref(self._scratch), C.c_size_t(nbytes)):
            raise RuntimeError("out of device memory for the resolved statistics")
        self.resolve(None if want_variance else self._scratch, self._scratch if want_variance else None)
        out = np.zeros((self.pixel_count, 4), np.float32)
        # (ordered behind the resolve on the device's stream)
        if self.lib.wait_for_device(C.byref(self.owner.app.device)) or self._hip.hipMemcpy(C.c_void_p(out.ctypes.data), self._scratch, C.c_size_t(nbytes), 2):
            raise RuntimeError("reading the resolved statistics back failed")
        return out

    def mean(self):
        return self._resolved(False)

    def variance(self):
        return self._resolved(True)

    def sums(self):
        """(S, Q): the accumulators as float64 arrays (pixels, 3)"""
        sums, squares = np.zeros((self.pixel_count, 3), np.float64), np.zeros((self.pixel_count, 3), np.float64)
        if self.lib.read_back_frame_statistics(C.byref(self.stats), C.byref(self.owner.app), sums.ctypes.data, squares.ctypes.data):
            raise RuntimeError("read_back_frame_statistics failed")
        return sums, squares

    def reset(self):
        if self.lib.reset_frame_statistics(C.byref(self.stats), C.byref(self.owner.app)):
            raise RuntimeError("reset_frame_statistics failed")

    def close(self):
        super().close()
        if self._scratch:
            self._hip.hipFree(self._scratch)
            self._scratch = C.c_void_p()


class _FrameImageObject(_FrameObject):
    """What FrameFilter and FrameHistory are: images of one extent on the device and a C function that takes settings and
    an images struct - the caller's inputs, then out_colour and out_variance."""
    # the C function, the struct of its images, a noun for messages and what the read-back of a result is called
    CALL = IMAGES = NOUN = RESULT = None

    def __init__(self, owner, width=None, height=None):
        super().__init__(owner, int(width or 0), int(height or 0))

    @property
    def width(self):
        return int(self.struct.width)

    @property
    def height(self):
        return int(self.struct.height)

    def _call(self, inputs, settings, out_colour, out_variance, want_variance, call=None, further=()):
        """inputs: device addresses, None or float32 arrays (height, width, 4), which are uploaded, in the order of the
        images struct; settings: the struct.  With out_colour the results stay on the device (out_variance too, if given)
        and the call gives nothing; else -> (colour, variance or None without want_variance) as arrays.  call: another C
        function than CALL, which takes the images `further`, given like inputs, behind the images struct."""
        call = call or self.CALL
        shape = (self.height, self.width, 4)
        nbytes = 16 * self.width * self.height
        with _DeviceScratch(self.owner, "an image of the %s" % self.NOUN, "an image of this %s" % self.NOUN) as scratch:
            def address(image):
                return scratch.upload(image, shape) if isinstance(image, np.ndarray) else (None if image is None else _address(image))
            images = self.IMAGES(*(address(image) for image in inputs))
            stays = out_colour is not None
            images.out_colour = _address(out_colour) if stays else scratch.allocate(nbytes)
            if out_variance is not None:
                images.out_variance = _address(out_variance)
            elif not stays and want_variance:
                images.out_variance = scratch.allocate(nbytes)
            if getattr(self.lib, call)(C.byref(self.struct), C.byref(self.owner.app), C.byref(settings), C.byref(images), *(address(image) for image in further)):
                raise RuntimeError("%s failed" % call)
            if stays:
                return None
            self.owner.sync()
            return tuple(scratch.download(address, shape, np.float32, "the %s image" % self.RESULT) if address else None for address in (images.out_colour, images.out_variance))


class FrameFilter(_FrameImageObject):
    """Renderer.create_frame_filter(): the scratch images and the event of filter_frame() for one extent"""
    NAME, STRUCT, ALIVE = "frame_filter", capi.FrameFilter, "filtered"
    CALL, IMAGES, NOUN, RESULT = "filter_frame", capi.FrameFilterImages, "filter", "filtered"

    def __init__(self, owner, width=None, height=None):
        super().__init__(owner, width, height)
        self.filter = self.struct

    def filter_settings(self, settings=None):
        from . import frame_filter
        values = dict(frame_filter.DEFAULT_SETTINGS, **(settings or {}))
        return capi.FrameFilterSettings(int(values["iteration_count"]), int(values["normal_squarings"]), float(values["sigma_luminance"]),
                                        float(values["sigma_depth"]), float(values["variance_scale"]))

    def apply(self, colour, variance, position, normal, modulation=None, settings=None, out_colour=None, out_variance=None):
        """See Renderer.filter_frame()"""
        return self._call((colour, variance, position, normal, modulation), self.filter_settings(settings), out_colour, out_variance, variance is not None)


class FrameHistory(_FrameImageObject):
    """Renderer.create_frame_history(): the two sets of history images and the event of accumulate_frame_history() for one
    extent"""
    NAME, STRUCT, ALIVE = "frame_history", capi.FrameHistory, "accumulated"
    CALL, IMAGES, NOUN, RESULT = "accumulate_frame_history", capi.FrameHistoryImages, "history", "accumulated"

    def __init__(self, owner, width=None, height=None):
        super().__init__(owner, width, height)
        self.history = self.struct

    @property
    def frame_count(self):
        return int(self.history.frame_count)

    def history_settings(self, settings=None):
        from . import frame_history
        values = dict(frame_history.DEFAULT_SETTINGS, **(settings or {}))
        return capi.FrameHistorySettings(float(values["max_length"]), float(values["sigma_depth"]), float(values["normal_threshold"]), int(values["spatial_length"]))

    def reset(self):
        """The next frame finds no history"""
        self.lib.reset_frame_history(C.byref(self.history))

    def read(self):
        """-> {"colour", "moments", "position", "normal"}: the set that the last call wrote, as arrays (height, width, 4)"""
        self.owner.sync()
        return {name: _DeviceScratch.download(getattr(self.history, name)[self.history.current], (self.height, self.width, 4), np.float32, "an image of the history")
                for name in ("colour", "moments", "position", "normal")}

    def accumulate(self, colour, features, settings=None, modulation=None, out_colour=None, out_variance=None, want_variance=True):
        """See Renderer.accumulate_history()"""
        if modulation is None:
            modulation = features.get("diffuse_albedo")
        inputs = (colour, features["position"], features["normal"], features.get("reprojection"), modulation)
        if features.get("previous_position") is None:
            return self._call(inputs, self.history_settings(settings), out_colour, out_variance, want_variance)
        return self._call(inputs, self.history_settings(settings), out_colour, out_variance, want_variance, "accumulate_moving_frame_history", (features["previous_position"],))


# ---- what the command lines share ---------------------------------------------------------------------------------

def add_dataset_arguments(parser, spp=True):
    parser.add_argument("dataset", help="directory of a dataset (scene.vks, LTC tables), as bench.py and the tests write it")
    parser.add_argument("--config", type=int, default=3)
    parser.add_argument("--width", type=int, default=None)
    parser.add_argument("--height", type=int, default=None)
    if spp:
        parser.add_argument("--spp", type=int, default=1, help="samples per pixel of a frame")


def add_output_arguments(parser):
    parser.add_argument("--out", metavar="DIR", required=True)
    output = parser.add_mutually_exclusive_group()
    output.add_argument("--hdr", action="store_true", help="Radiance files through the device's encoder (the default)")
    output.add_argument("--png", action="store_true", help="PNG files of the sRGB8 encoding through the device's encoder")


def dataset_of(directory):
    """What renderer.setup_config() takes of a dataset's directory"""
    ltc = os.path.join(directory, "ltc")
    return {"scene": os.path.join(directory, "scene.vks"), "textures": os.path.join(directory, "textures"), "ltc": ltc,
            "fresnel_count": len([name for name in os.listdir(ltc) if name.startswith("fit")])}


@contextlib.contextmanager
def open_dataset(options, animate_noise=False, **overrides):
    """A Renderer with the dataset, the configuration and the extent of the options, its targets and its pass; closed on
    the way out"""
    from . import renderer
    scene = renderer.Renderer()
    try:
        renderer.setup_config(scene, options.config, dataset_of(options.dataset), width=options.width, height=options.height, acceleration_structure=True, **overrides)
        if animate_noise:
            scene.app.render_settings.animate_noise = 1
        scene.create_targets()
        scene.create_pass()
        yield scene
    finally:
        scene.close()


def write_images(scene, scratch, options, images):
    """Writes (name, device address) pairs of float frames as <out>/<name>.hdr or, with --png, as .png files"""
    extent = scene.app.swapchain.extent
    pixels = extent.width * extent.height
    encoded = scratch.allocate(16 * pixels)
    for name, image in images:
        if options.png:
            scene.encode_slab(image, encoded, pixels)
            data, suffix = scene.encode_png(encoded, width=extent.width, height=extent.height), ".png"
        else:
            data, suffix = scene.encode_hdr(image, width=extent.width, height=extent.height), ".hdr"
        path = os.path.join(options.out, name + suffix)
        with open(path, "wb") as file:
            file.write(data)
        print("%s -> %s (%d bytes)" % (name, path, len(data)))
