"""ctypes mirror of include/pngloss_hip.h (the drop-in seam of /root/reference/src/pngloss_image.h:14-29)."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
_ROOT = os.path.dirname(_HERE)

#: libpng filter flag values written to row_filters (pngloss_image.c:290-306): none, sub, up, average, paeth
PNG_FILTER_FLAGS = (0x08, 0x10, 0x20, 0x40, 0x80)

PNGLOSS_SUCCESS = 0
PNGLOSS_INVALID_ARGUMENT = 4
PNGLOSS_OUT_OF_MEMORY_ERROR = 17
PNGLOSS_HIP_ERROR = 64
PNGLOSS_INTERNAL_ABORT = 65

_lock = threading.Lock()
_hip = None
_synth = None


# ---- the header's structs (STRUCTS below names them; tests/test_abi.py compares every size and offset with the compiler's) ----------

class PnglossImage(C.Structure):
    _fields_ = [("rows", C.POINTER(C.c_void_p)), ("width", C.c_uint32), ("height", C.c_uint32),
                ("bytes_per_pixel", C.c_uint8)]


class ImageDesc(C.Structure):
    _fields_ = [("d_rgba", C.c_void_p), ("d_row_filters", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32)]


class HostImage(C.Structure):
    _fields_ = [("rgba", C.c_void_p), ("row_filters", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32)]


class Scanlines(C.Structure):
    _fields_ = [("filter_types", C.c_void_p), ("scanlines", C.c_void_p), ("pitch", C.c_size_t), ("color_type", C.c_int)]


class ZStream(C.Structure):
    _fields_ = [("data", C.c_void_p), ("capacity", C.c_size_t), ("size", C.c_size_t), ("color_type", C.c_int),
                ("blocks", C.c_uint32 * 3), ("flags", C.c_uint32)]


class PngSource(C.Structure):
    """pngloss_hip_png_source.  `interlace` (0 = none, 1 = Adam7) sits in what was padding behind bit_depth; the positional arguments are the
    ten of the struct without it, so it is given by keyword."""
    _fields_ = [("scanlines", C.c_char_p), ("width", C.c_uint32), ("height", C.c_uint32), ("color_type", C.c_uint8), ("bit_depth", C.c_uint8),
                ("interlace", C.c_uint8),
                ("palette", C.c_char_p), ("palette_entries", C.c_uint32), ("trns", C.c_char_p), ("trns_bytes", C.c_uint32), ("rgba", C.c_void_p)]

    def __init__(self, scanlines=None, width=0, height=0, color_type=0, bit_depth=0, palette=None, palette_entries=0, trns=None, trns_bytes=0,
                 rgba=None, interlace=0):
        super().__init__(scanlines, width, height, color_type, bit_depth, interlace, palette, palette_entries, trns, trns_bytes, rgba)


class PngZSource(C.Structure):
    """pngloss_hip_png_zsource; `interlace` by keyword, as in PngSource."""
    _fields_ = [("zstream", C.c_char_p), ("zbytes", C.c_size_t), ("width", C.c_uint32), ("height", C.c_uint32), ("color_type", C.c_uint8), ("bit_depth", C.c_uint8),
                ("interlace", C.c_uint8),
                ("palette", C.c_char_p), ("palette_entries", C.c_uint32), ("trns", C.c_char_p), ("trns_bytes", C.c_uint32)]

    def __init__(self, zstream=None, zbytes=0, width=0, height=0, color_type=0, bit_depth=0, palette=None, palette_entries=0, trns=None, trns_bytes=0,
                 interlace=0):
        super().__init__(zstream, zbytes, width, height, color_type, bit_depth, interlace, palette, palette_entries, trns, trns_bytes)


class Result(C.Structure):
    _fields_ = [("status", C.c_int32), ("bytes_per_pixel", C.c_uint32), ("unique_symbols", C.c_uint32),
                ("retried_rows", C.c_uint32), ("repaired_pixels", C.c_uint32)]


class Distortion(C.Structure):
    """pngloss_hip_distortion: how far a result is from its original (a = original, b = result; channels R, G, B, A).  All exact integers."""
    _fields_ = [("pixels", C.c_uint64), ("changed_pixels", C.c_uint64), ("sq_err", C.c_uint64 * 4), ("max_abs", C.c_uint32 * 4)]

    def as_dict(self):
        return dict(pixels=self.pixels, changed_pixels=self.changed_pixels, sq_err=list(self.sq_err), max_abs=list(self.max_abs))

    def psnr_db(self, channel_mask=0xF):
        return psnr_db(self, channel_mask)


class Ssim(C.Structure):
    """pngloss_hip_ssim: the structural similarity of a result to its original over 8x8 windows at a stride of 4 (channels R, G, B, A).  All exact
    integers: sum_q16[c] is the sum and min_q16[c] the smallest of the windows' q (65536 = equal windows)."""
    _fields_ = [("windows", C.c_uint64), ("sum_q16", C.c_int64 * 4), ("min_q16", C.c_int32 * 4), ("reserved", C.c_uint64)]

    def as_dict(self):
        return dict(windows=self.windows, sum_q16=list(self.sum_q16), min_q16=list(self.min_q16), reserved=self.reserved)

    def mean(self, channel_mask=0xF):
        return ssim_mean(self, channel_mask)


class Palette(C.Structure):
    """pngloss_hip_palette: what the option "indexed" decided for one image and from which numbers.  entries == 0: written as truecolour; else the
    stream is colour type 3 and rgb[:entries] / alpha[:trns_entries] are its PLTE / tRNS payloads.  colors: 257 = more than 256."""
    _fields_ = [("entries", C.c_uint32), ("trns_entries", C.c_uint32), ("rgb", (C.c_uint8 * 3) * 256), ("alpha", C.c_uint8 * 256),
                ("truecolor_bytes", C.c_uint64), ("indexed_bytes", C.c_uint64), ("colors", C.c_uint32), ("reserved", C.c_uint32)]

    def plte(self):
        return bytes(bytearray(self.rgb)[: 3 * self.entries])

    def trns(self):
        return bytes(bytearray(self.alpha)[: self.trns_entries])

    def as_dict(self):
        return dict(entries=self.entries, trns_entries=self.trns_entries, plte=self.plte(), trns=self.trns(), truecolor_bytes=self.truecolor_bytes,
                    indexed_bytes=self.indexed_bytes, colors=self.colors)


class IndexDepth(C.Structure):
    """pngloss_hip_index_depth: which bit depth the option "index_depth" kept for one image (0: truecolour) and from which sizes.  min_depth: 1, 2,
    4 or 8 for an eligible image, else 0; indexed8_bytes / packed_bytes: 0 where that candidate was not written."""
    _fields_ = [("bit_depth", C.c_uint32), ("min_depth", C.c_uint32), ("indexed8_bytes", C.c_uint64), ("packed_bytes", C.c_uint64)]

    def as_dict(self):
        return dict(bit_depth=self.bit_depth, min_depth=self.min_depth, indexed8_bytes=self.indexed8_bytes, packed_bytes=self.packed_bytes)


class QuantParams(C.Structure):
    """pngloss_hip_quant_params: max_colors (N, 2..256) and rounds (R, 0..64) of the colour quantiser.  include/pngloss_hip_quant.h states the rule."""
    _fields_ = [("max_colors", C.c_uint32), ("rounds", C.c_uint32)]

    def __init__(self, max_colors=256, rounds=8):
        super().__init__(max_colors, rounds)


class QuantParams2(C.Structure):
    """pngloss_hip_quant_params2: QuantParams with dither (DITHER_NONE = 0, DITHER_FLOYD_STEINBERG = 1) and reserved (0).
    include/pngloss_hip_dither.h states the rule."""
    _fields_ = [("max_colors", C.c_uint32), ("rounds", C.c_uint32), ("dither", C.c_uint32), ("reserved", C.c_uint32)]

    def __init__(self, max_colors=256, rounds=8, dither=0, reserved=0):
        super().__init__(max_colors, rounds, dither, reserved)


class QuantParams3(C.Structure):
    """pngloss_hip_quant_params3: QuantParams2 with its last word named: space (QUANT_SPACE_RGBA = 0, QUANT_SPACE_VISIBLE = 1: the palette search
    runs on alpha-premultiplied pixels).  include/pngloss_hip_quant_space.h states the rule."""
    _fields_ = [("max_colors", C.c_uint32), ("rounds", C.c_uint32), ("dither", C.c_uint32), ("space", C.c_uint32)]

    def __init__(self, max_colors=256, rounds=8, dither=0, space=0):
        super().__init__(max_colors, rounds, dither, space)


class QuantReport(C.Structure):
    """pngloss_hip_quant_report: what the quantiser did to one image.  colors_in: 257 = more than 256; palette[:entries]: the colours of the image as
    it is now, ascending by word; exact: it had at most max_colors colours and was not changed; distortion: now against the input, all pixels."""
    _fields_ = [("status", C.c_int32), ("colors_in", C.c_uint32), ("entries", C.c_uint32), ("exact", C.c_uint32), ("palette", C.c_uint32 * 256),
                ("distortion", Distortion)]

    def as_dict(self):
        return dict(status=self.status, colors_in=self.colors_in, entries=self.entries, exact=self.exact, palette=list(self.palette)[: self.entries],
                    distortion=self.distortion.as_dict())


class QuantTarget(C.Structure):
    """pngloss_hip_quant_target: min_psnr_db (0 = no condition, inf = only exact results pass) and max_abs_error (0 = no condition, 1..255); one
    of the two has to be set.  include/pngloss_hip_quant_target.h states the rule."""
    _fields_ = [("min_psnr_db", C.c_double), ("max_abs_error", C.c_uint32), ("reserved", C.c_uint32)]

    def __init__(self, min_psnr_db=0.0, max_abs_error=0, reserved=0):
        super().__init__(min_psnr_db, max_abs_error, reserved)


class QuantTargetReport(C.Structure):
    """pngloss_hip_quant_target_report: the chosen colour count, whether the target was reached, the probes of the rule (probed[k] and bit k of
    accepted_mask), the Distortion the probe at `colors` took and the QuantReport of pngloss_hip_quantize_batch2 at `colors`."""
    _fields_ = [("colors", C.c_uint32), ("reached", C.c_uint32), ("probes", C.c_uint32), ("accepted_mask", C.c_uint32), ("probed", C.c_uint32 * 12),
                ("probe_distortion", Distortion), ("quant", QuantReport)]

    def as_dict(self):
        return dict(colors=self.colors, reached=self.reached, probes=self.probes, accepted_mask=self.accepted_mask, probed=list(self.probed)[: self.probes],
                    probe_distortion=self.probe_distortion.as_dict(), quant=self.quant.as_dict())


class ImagePair(C.Structure):
    _fields_ = [("d_a", C.c_void_p), ("d_b", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32)]


class Target(C.Structure):
    """pngloss_hip_target: min_psnr_db (0 = no condition, inf = only lossless results pass), max_abs_error (0 = no condition, 1..255) and
    max_strength (M, 0..255: the search never goes above it).  include/pngloss_hip.h states the rule."""
    _fields_ = [("min_psnr_db", C.c_double), ("max_abs_error", C.c_uint32), ("max_strength", C.c_uint32)]

    def __init__(self, min_psnr_db=0.0, max_abs_error=0, max_strength=19):
        super().__init__(min_psnr_db, max_abs_error, max_strength)


class Target2(C.Structure):
    """pngloss_hip_target2: a Target with min_ssim, the smallest allowed mean SSIM over the stored channels (0 = no condition, else in (0, 1])."""
    _fields_ = [("min_psnr_db", C.c_double), ("max_abs_error", C.c_uint32), ("max_strength", C.c_uint32), ("min_ssim", C.c_double)]

    def __init__(self, min_psnr_db=0.0, max_abs_error=0, max_strength=19, min_ssim=0.0):
        super().__init__(min_psnr_db, max_abs_error, max_strength, min_ssim)


class TargetReport(C.Structure):
    """pngloss_hip_target_report: the chosen strength, the probes of the rule, the row-engine runs spent and the Distortion of the result kept."""
    _fields_ = [("strength", C.c_uint32), ("probes", C.c_uint32), ("runs", C.c_uint32), ("reserved", C.c_uint32), ("distortion", Distortion)]

    def as_dict(self):
        return dict(strength=self.strength, probes=self.probes, runs=self.runs, distortion=self.distortion.as_dict())


class SizeTarget(C.Structure):
    """pngloss_hip_size_target: max_bytes (one budget per image: the largest allowed zlib stream) and max_strength (M, 0..255: the search never
    goes above it).  include/pngloss_hip.h states the rule.  max_bytes: a ctypes array of c_uint64, a sequence of ints, or None."""
    _fields_ = [("max_bytes", C.POINTER(C.c_uint64)), ("max_strength", C.c_uint32), ("reserved", C.c_uint32)]

    def __init__(self, max_bytes=None, max_strength=19):
        if max_bytes is not None and not isinstance(max_bytes, C.Array):
            max_bytes = (C.c_uint64 * max(len(max_bytes), 1))(*max_bytes)
        self._budgets = max_bytes                          # (keeps the array alive)
        super().__init__(C.cast(max_bytes, C.POINTER(C.c_uint64)) if max_bytes is not None else None, max_strength, 0)


class SizeReport(C.Structure):
    """pngloss_hip_size_report: the chosen strength, the probes of the rule, the row-engine runs spent, whether the budget was reached, the measured
    stream size and colour type of the result kept, and its Distortion."""
    _fields_ = [("strength", C.c_uint32), ("probes", C.c_uint32), ("runs", C.c_uint32), ("reached", C.c_uint32), ("bytes", C.c_uint64),
                ("color_type", C.c_int32), ("reserved", C.c_uint32), ("distortion", Distortion)]

    def as_dict(self):
        return dict(strength=self.strength, probes=self.probes, runs=self.runs, reached=self.reached, bytes=self.bytes, color_type=self.color_type,
                    distortion=self.distortion.as_dict())


#: the header's name of every struct it defines -> its mirror above
STRUCTS = {
    "pngloss_image": PnglossImage, "pngloss_hip_image_desc": ImageDesc, "pngloss_hip_result": Result, "pngloss_hip_host_image": HostImage,
    "pngloss_hip_scanlines": Scanlines, "pngloss_hip_zstream": ZStream, "pngloss_hip_distortion": Distortion, "pngloss_hip_image_pair": ImagePair,
    "pngloss_hip_ssim": Ssim, "pngloss_hip_target": Target, "pngloss_hip_target_report": TargetReport, "pngloss_hip_target2": Target2,
    "pngloss_hip_size_target": SizeTarget, "pngloss_hip_size_report": SizeReport, "pngloss_hip_png_source": PngSource,
    "pngloss_hip_png_zsource": PngZSource,
}

#: the same two tables for include/pngloss_hip_indexed.h, the extension header of the option "indexed" (tests/test_index_host.py holds them
#: against that header the way tests/test_abi.py holds STRUCTS and PROTOTYPES against pngloss_hip.h)
INDEXED_STRUCTS = {"pngloss_hip_palette": Palette}
INDEXED_PROTOTYPES = {
    "pngloss_hip_last_palette": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(Palette)]),
    "pngloss_hip_multi_last_palette": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(Palette)]),
}


#: ... and for include/pngloss_hip_quant.h, the extension header of the colour quantiser (tests/test_quant_host.py holds them against that header)
QUANT_STRUCTS = {"pngloss_hip_quant_params": QuantParams, "pngloss_hip_quant_report": QuantReport}
QUANT_PROTOTYPES = {
    "pngloss_hip_quantize_batch": (C.c_int, [C.c_void_p, C.POINTER(ImageDesc), C.c_size_t, C.POINTER(QuantParams), C.POINTER(QuantReport), C.c_void_p]),
    "pngloss_hip_multi_quantize_batch_host": (C.c_int, [C.c_void_p, C.POINTER(HostImage), C.c_size_t, C.POINTER(QuantParams), C.POINTER(QuantReport)]),
}

#: ... and for include/pngloss_hip_dither.h, the dithering extension of the quantiser (tests/test_dither_host.py holds them against that header)
DITHER_NONE, DITHER_FLOYD_STEINBERG = 0, 1
DITHER_STRUCTS = {"pngloss_hip_quant_params2": QuantParams2}
DITHER_PROTOTYPES = {
    "pngloss_hip_quantize_batch2": (C.c_int, [C.c_void_p, C.POINTER(ImageDesc), C.c_size_t, C.POINTER(QuantParams2), C.POINTER(QuantReport), C.c_void_p]),
    "pngloss_hip_multi_quantize_batch_host2": (C.c_int, [C.c_void_p, C.POINTER(HostImage), C.c_size_t, C.POINTER(QuantParams2), C.POINTER(QuantReport)]),
}

#: ... and for include/pngloss_hip_quant_target.h, the quantiser's colour count from a distortion target (tests/test_quant_target_host.py holds
#: them against that header)
QUANT_TARGET_STRUCTS = {"pngloss_hip_quant_target": QuantTarget, "pngloss_hip_quant_target_report": QuantTargetReport}
QUANT_TARGET_PROTOTYPES = {
    "pngloss_hip_quantize_batch_target": (C.c_int, [C.c_void_p, C.POINTER(ImageDesc), C.c_size_t, C.POINTER(QuantParams2), C.POINTER(QuantTarget),
                                                    C.POINTER(QuantTargetReport), C.c_void_p]),
    "pngloss_hip_multi_quantize_batch_host_target": (C.c_int, [C.c_void_p, C.POINTER(HostImage), C.c_size_t, C.POINTER(QuantParams2), C.POINTER(QuantTarget),
                                                               C.POINTER(QuantTargetReport)]),
}

#: ... and for include/pngloss_hip_quant_space.h, the quantiser's calls with the space of the palette search (tests/test_quant_space_host.py holds
#: them against that header)
QUANT_SPACE_RGBA, QUANT_SPACE_VISIBLE = 0, 1
QUANT_SPACE_STRUCTS = {"pngloss_hip_quant_params3": QuantParams3}
QUANT_SPACE_PROTOTYPES = {
    "pngloss_hip_quantize_batch3": (C.c_int, [C.c_void_p, C.POINTER(ImageDesc), C.c_size_t, C.POINTER(QuantParams3), C.POINTER(QuantReport), C.c_void_p]),
    "pngloss_hip_multi_quantize_batch_host3": (C.c_int, [C.c_void_p, C.POINTER(HostImage), C.c_size_t, C.POINTER(QuantParams3), C.POINTER(QuantReport)]),
    "pngloss_hip_quantize_batch_target3": (C.c_int, [C.c_void_p, C.POINTER(ImageDesc), C.c_size_t, C.POINTER(QuantParams3), C.POINTER(QuantTarget),
                                                     C.POINTER(QuantTargetReport), C.c_void_p]),
    "pngloss_hip_multi_quantize_batch_host_target3": (C.c_int, [C.c_void_p, C.POINTER(HostImage), C.c_size_t, C.POINTER(QuantParams3), C.POINTER(QuantTarget),
                                                                C.POINTER(QuantTargetReport)]),
}

#: ... and for include/pngloss_hip_index_depth.h, the bit depths of the indexed-colour write side (tests/test_index_depth_host.py holds them against
#: that header)
INDEX_DEPTH_STRUCTS = {"pngloss_hip_index_depth": IndexDepth}
INDEX_DEPTH_PROTOTYPES = {
    "pngloss_hip_last_index_depth": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(IndexDepth)]),
    "pngloss_hip_multi_last_index_depth": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(IndexDepth)]),
}


def _prototypes():
    """name -> (restype, [argtypes]) for every function include/pngloss_hip.h declares, in the header's order"""
    ptr, vp, cp, sz, i, u, lg, dbl, u32 = C.POINTER, C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.c_uint, C.c_long, C.c_double, C.c_uint32
    quant = [C.c_bool, C.c_uint8, lg]                                        # verbose, quantization_strength, bleed_divider of the seam
    device = [vp, ptr(ImageDesc), sz]                                        # ctx, images, n
    host = [vp, ptr(HostImage), sz]                                          # ctx or multi, images, n
    res, lines, zs = ptr(Result), ptr(Scanlines), ptr(ZStream)
    decoded = [ptr(vp), ptr(i), vp]                                          # d_rgba, status, stream
    return {
        "optimize_with_rows": (i, [ptr(vp), u32, u32, vp] + quant),
        "optimize_with_stride": (None, [vp, u32, u32, u32] + quant),
        "optimizeForAverageFilter": (None, [vp, i, i, i]),
        "optimize_image": (i, [ptr(PnglossImage), vp] + quant),
        "pngloss_hip_device_count": (i, []),
        "pngloss_hip_create": (vp, [i]),
        "pngloss_hip_destroy": (None, [vp]),
        "pngloss_hip_optimize_batch_async": (i, device + [u, lg, vp]),
        "pngloss_hip_finish": (i, [vp, res, sz]),
        "pngloss_hip_optimize_batch": (i, device + [u, lg, vp, res]),
        "pngloss_hip_optimize_batch_host": (i, host + [u, lg, res]),
        "pngloss_hip_multi_create": (vp, [cp]),
        "pngloss_hip_multi_destroy": (None, [vp]),
        "pngloss_hip_multi_count": (i, [vp]),
        "pngloss_hip_multi_split": (None, [ptr(HostImage), sz, i, ptr(i)]),
        "pngloss_hip_optimize_batch_host_emit": (i, host + [u, lg, res, lines]),
        "pngloss_hip_zlib_bound": (sz, [u32, u32]),
        "pngloss_hip_multi_optimize_batch_host": (i, host + [u, lg, res, lines, zs]),
        "pngloss_hip_optimize_batch_host_zlib": (i, host + [u, lg, res, zs]),
        "pngloss_hip_last_deflate_ms": (dbl, [vp]),
        "pngloss_hip_last_engine_ms": (dbl, [vp]),
        "pngloss_hip_last_total_ms": (dbl, [vp]),
        "pngloss_hip_last_histogram": (i, [vp, sz, vp]),
        "pngloss_hip_last_original_tables": (i, [vp, sz, vp, vp]),
        "pngloss_hip_last_distortion": (i, [vp, sz, ptr(Distortion)]),
        "pngloss_hip_compare_batch": (i, [vp, ptr(ImagePair), sz, ptr(Distortion), vp]),
        "pngloss_hip_psnr_db": (dbl, [ptr(Distortion), u]),
        "pngloss_hip_multi_set_option": (i, [vp, cp, cp]),
        "pngloss_hip_multi_last_distortion": (i, [vp, sz, ptr(Distortion)]),
        "pngloss_hip_last_ssim": (i, [vp, sz, ptr(Ssim)]),
        "pngloss_hip_multi_last_ssim": (i, [vp, sz, ptr(Ssim)]),
        "pngloss_hip_compare_batch_ssim": (i, [vp, ptr(ImagePair), sz, ptr(Ssim), vp]),
        "pngloss_hip_ssim_mean": (dbl, [ptr(Ssim), u]),
        "pngloss_hip_compare_batch_visible": (i, [vp, ptr(ImagePair), sz, ptr(Distortion), ptr(Ssim), vp]),
        "pngloss_hip_optimize_batch_target": (i, device + [ptr(Target), lg, vp, res, ptr(TargetReport)]),
        "pngloss_hip_multi_optimize_batch_host_target": (i, host + [ptr(Target), lg, res, lines, zs, ptr(TargetReport)]),
        "pngloss_hip_optimize_batch_target2": (i, device + [ptr(Target2), lg, vp, res, ptr(TargetReport), ptr(Ssim)]),
        "pngloss_hip_multi_optimize_batch_host_target2": (i, host + [ptr(Target2), lg, res, lines, zs, ptr(TargetReport), ptr(Ssim)]),
        "pngloss_hip_optimize_batch_size": (i, device + [ptr(SizeTarget), lg, vp, res, zs, ptr(SizeReport)]),
        "pngloss_hip_multi_optimize_batch_host_size": (i, host + [ptr(SizeTarget), lg, res, lines, zs, ptr(SizeReport)]),
        "pngloss_hip_png_decode_batch_host": (i, [vp, ptr(PngSource), sz]),
        "pngloss_hip_png_decode_batch_host_status": (i, [vp, ptr(PngSource), sz, ptr(i)]),
        "pngloss_hip_png_decode_batch_device": (i, [vp, ptr(PngSource), sz] + decoded),
        "pngloss_hip_png_decode_batch_device_z": (i, [vp, ptr(PngZSource), sz] + decoded),
        "pngloss_hip_pinned_alloc": (vp, [sz]),
        "pngloss_hip_pinned_free": (None, [vp]),
        "pngloss_hip_last_engine_info": (i, [vp, sz, vp]),
        "pngloss_hip_set_option": (i, [vp, cp, cp]),
        "pngloss_hip_version": (cp, []),
    }


#: the C ABI as ctypes sees it; hip_lib() applies it when it loads the library, and tests/test_abi.py checks every entry (return class, argument
#: count, each argument's class) against the header's declarations, as it checks STRUCTS against the header's layouts
PROTOTYPES = _prototypes()

#: every symbol include/pngloss_hip.h declares (tests/test_host_logic.py checks the names against the header and that the .so exports each)
ABI_SYMBOLS = tuple(PROTOTYPES)

#: the channels an image of `bytes_per_pixel` 1..4 stores (gray is the G channel): the mask pngloss_hip_psnr_db takes for it
PSNR_MASK_OF_BPP = {1: 0x2, 2: 0xA, 3: 0x7, 4: 0xF}


def parse_png(data):
    """Chunk walk + inflate of a PNG file (what pngloss_amd/cli/png_stream_reader.c does in C with zlib): dict(width, height, depth, ctype,
    interlace, plte, trns, zstream, scanlines)."""
    import struct
    import zlib
    data = bytes(data)
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("not a PNG file")
    o, out, idat = 8, dict(plte=None, trns=None), []
    while o + 8 <= len(data):
        n, tag = struct.unpack(">I4s", data[o:o + 8])
        body = data[o + 8:o + 8 + n]
        o += 12 + n
        if tag == b"IHDR":
            out["width"], out["height"], out["depth"], out["ctype"], _, _, out["interlace"] = struct.unpack(">IIBBBBB", body)
        elif tag == b"PLTE":
            out["plte"] = body
        elif tag == b"tRNS":
            out["trns"] = body
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            break
    out["zstream"] = b"".join(idat)
    out["scanlines"] = zlib.decompress(out["zstream"])
    return out


def psnr_db(distortion, channel_mask=0xF):
    """pngloss_hip_psnr_db: 10 log10(255^2 * pixels * popcount(mask) / sum of sq_err over the mask's channels); inf for a sum of 0, nan for no
    pixels or a mask outside 1..15.  `distortion`: a Distortion or the dict Distortion.as_dict() gives.  Host arithmetic: needs no GPU."""
    if not isinstance(distortion, Distortion):
        d = distortion
        distortion = Distortion(d["pixels"], d["changed_pixels"], (C.c_uint64 * 4)(*d["sq_err"]), (C.c_uint32 * 4)(*d["max_abs"]))
    return hip_lib().pngloss_hip_psnr_db(C.byref(distortion), channel_mask)


def ssim_mean(ssim, channel_mask=0xF):
    """pngloss_hip_ssim_mean: the sum of sum_q16 over the mask's channels / (65536 * windows * popcount(mask)); nan for no windows or a mask outside
    1..15.  `ssim`: an Ssim or the dict Ssim.as_dict() gives.  Host arithmetic: needs no GPU."""
    if not isinstance(ssim, Ssim):
        d = ssim
        ssim = Ssim(d["windows"], (C.c_int64 * 4)(*d["sum_q16"]), (C.c_int32 * 4)(*d["min_q16"]), d.get("reserved", 0))
    return hip_lib().pngloss_hip_ssim_mean(C.byref(ssim), channel_mask)


def build(verbose: bool = False) -> None:
    """Compile libpngloss_hip.so (hipcc, gfx950) and libpngloss_synth.so (gcc) in-tree."""
    r = subprocess.run(["make", "-C", _CSRC, "-j4"], capture_output=True, text=True)
    if verbose or r.returncode:
        print(r.stdout[-4000:])
        print(r.stderr[-4000:])
    if r.returncode:
        raise RuntimeError("building pngloss_amd/csrc failed")


def _load(name):
    path = os.path.join(_CSRC, name)
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback for the HIP path)")
    return C.CDLL(path)


def synth_lib():
    global _synth
    with _lock:
        if _synth is None:
            lib = _load("libpngloss_synth.so")
            lib.pngloss_synth_rgba.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint64]
            lib.pngloss_synth_rgba.restype = None
            lib.pngloss_fnv1a64.argtypes = [C.c_void_p, C.c_size_t]
            lib.pngloss_fnv1a64.restype = C.c_uint64
            lib.pngloss_fnv1a64_seed.argtypes = [C.c_void_p, C.c_size_t, C.c_uint64]
            lib.pngloss_fnv1a64_seed.restype = C.c_uint64
            _synth = lib
        return _synth


def hip_lib():
    global _hip
    with _lock:
        if _hip is None:
            # PyTorch-ROCm wheels bundle their own libamdhip64; whichever copy is loaded first serves the whole process.
            # Loading /opt/rocm's copy first (through our .so) and torch's afterwards leaves torch without devices, so
            # when torch is installed let it load first.  The C library itself has no torch dependency.
            if "torch" not in sys.modules and os.environ.get("PNGLOSS_NO_TORCH_PRELOAD") is None:
                try:
                    import torch  # noqa: F401
                except ImportError:
                    pass
            lib = _load(os.environ.get("PNGLOSS_HIP_LIBNAME", "libpngloss_hip.so"))
            for name, (ret, args) in {**PROTOTYPES, **INDEXED_PROTOTYPES, **QUANT_PROTOTYPES, **DITHER_PROTOTYPES, **QUANT_TARGET_PROTOTYPES,
                                       **QUANT_SPACE_PROTOTYPES, **INDEX_DEPTH_PROTOTYPES}.items():
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = ret, args
            _hip = lib
        return _hip


def _check(rc, what, partial_ok=False):
    """partial_ok: the batch entry points return PNGLOSS_INTERNAL_ABORT (65) when SINGLE images hit the row the reference abort()s on
    (pngloss_image.c:268-271) -- every other image of the batch is done and results[i].status tells which failed, so the wrappers
    hand the per-image statuses back instead of throwing the whole batch away."""
    if rc != PNGLOSS_SUCCESS and not (partial_ok and rc == PNGLOSS_INTERNAL_ABORT):
        raise RuntimeError(f"{what} failed with pngloss_error {rc}")


# ---- marshalling: each table of the C ABI is filled in one place, and read back in one place ----------------------------------------------------
# The arrays a helper returns beside a table are what the table points into: the caller keeps them in locals until the C call has returned.

def _array(ctype, n):
    """n elements of ctype; one for n = 0, so that an empty batch still hands the C side a valid pointer"""
    return (ctype * max(n, 1))()


def _row_pointers(arr: np.ndarray):
    h = arr.shape[0]
    stride = arr.strides[0]
    base = arr.ctypes.data
    return (C.c_void_p * max(h, 1))(*[base + y * stride for y in range(h)])


def _image_descs(images):
    """(d_rgba_ptr, d_filters_ptr_or_0, width, height) tuples -> ImageDesc table"""
    descs = _array(ImageDesc, len(images))
    for i, (p, f, w, h) in enumerate(images):
        descs[i] = ImageDesc(p or None, f or None, w, h)
    return descs


def _image_pairs(pairs):
    """(d_a_ptr, d_b_ptr, width, height) tuples -> ImagePair table"""
    arr = _array(ImagePair, len(pairs))
    for i, (a, b, w, h) in enumerate(pairs):
        arr[i] = ImagePair(a or None, b or None, w, h)
    return arr


def _host_images(arrays, want_filters=True, inplace=False):
    """(H, W, 4) uint8 arrays -> (outs, filts, HostImage table).  outs: copies for the C call to rewrite, or with inplace the arrays themselves
    (C-contiguous uint8); filts: one zeroed (H,) array each, or None each without want_filters (the table then carries NULL)."""
    outs = list(arrays) if inplace else [np.ascontiguousarray(a).copy() for a in arrays]
    if inplace:
        assert all(a.flags["C_CONTIGUOUS"] and a.dtype == np.uint8 for a in outs)
    filts = [np.zeros(a.shape[0], np.uint8) if want_filters else None for a in outs]
    imgs = _array(HostImage, len(outs))
    for i, (a, f) in enumerate(zip(outs, filts)):
        imgs[i] = HostImage(a.ctypes.data, f.ctypes.data if f is not None else None, a.shape[1], a.shape[0])
    return outs, filts, imgs


def _scanline_buffers(outs):
    """room for the filtered scanlines of every array of outs -> (Scanlines table, ids, rows): ids[i] (H,), rows[i] (H, W * 4), the pitch RGBA's"""
    ids = [np.zeros(a.shape[0], np.uint8) for a in outs]
    rows = [np.zeros((a.shape[0], a.shape[1] * 4), np.uint8) for a in outs]
    lines = _array(Scanlines, len(outs))
    for i, (f, r) in enumerate(zip(ids, rows)):
        lines[i] = Scanlines(f.ctypes.data, r.ctypes.data, r.shape[1], -1)
    return lines, ids, rows


def _scanlines_back(lines, ids, rows):
    """per image (color_type, filter_types[H], scanlines[H, W * channels]): the colour type the call detected says how much of a row it wrote"""
    channels = {0: 1, 4: 2, 2: 3, 6: 4}
    return [(lines[i].color_type, f, r[:, : r.shape[1] // 4 * channels.get(lines[i].color_type, 4)].copy()) for i, (f, r) in enumerate(zip(ids, rows))]


def _zstreams(lib, shapes, stream_only=False):
    """room for the zlib stream of every (width, height) of shapes -> (ZStream table, bufs); stream_only: PNGLOSS_HIP_Z_STREAM_ONLY"""
    bufs = [np.zeros(lib.pngloss_hip_zlib_bound(w, h), np.uint8) for (w, h) in shapes]
    zs = _array(ZStream, len(bufs))
    for i, b in enumerate(bufs):
        zs[i] = ZStream(b.ctypes.data, b.size, 0, -1, (C.c_uint32 * 3)(0, 0, 0), 1 if stream_only else 0)
    return zs, bufs


def _zstreams_back(zs, bufs):
    """per image (color_type, zlib stream bytes, blocks)"""
    return [(zs[i].color_type, b[: zs[i].size].tobytes(), tuple(zs[i].blocks)) for i, b in enumerate(bufs)]


def _shapes(arrays):
    return [(a.shape[1], a.shape[0]) for a in arrays]


def _png_chunks(p):
    """the palette and tRNS members both source structs end their common part with, from a parse_png dict"""
    return p["plte"], len(p["plte"]) // 3 if p["plte"] else 0, p["trns"], len(p["trns"]) if p["trns"] else 0


def _png_sources(parsed, outs=None, scanlines=None):
    """parse_png dicts -> PngSource table.  outs: the (H, W, 4) arrays the host forms decode into (the device forms use no rgba);
    scanlines: what to send in place of the parsed files' own (page-locked copies)."""
    src = _array(PngSource, len(parsed))
    for i, p in enumerate(parsed):
        src[i] = PngSource(scanlines[i] if scanlines is not None else p["scanlines"], p["width"], p["height"], p["ctype"], p["depth"], *_png_chunks(p),
                           outs[i].ctypes.data if outs is not None else None, interlace=p["interlace"])
    return src


def _decode_outputs(parsed):
    return [np.zeros((p["height"], p["width"], 4), np.uint8) for p in parsed]


def _frames(ptrs, parsed):
    return [(ptrs[i], p["width"], p["height"]) for i, p in enumerate(parsed)]


def _result_dict(r):
    """what the device-resident calls report per image"""
    return dict(status=r.status, bpp=r.bytes_per_pixel, unique_symbols=r.unique_symbols, retried_rows=r.retried_rows, repaired_pixels=r.repaired_pixels)


def _host_result_dict(r):
    """what the host-memory calls report per image"""
    return dict(status=r.status, bpp=r.bytes_per_pixel, unique_symbols=r.unique_symbols)


# ---- host-pointer seam, same names as the reference ---------------------------------------------------------

def optimize_with_rows(rgba: np.ndarray, strength: int = 19, bleed: int = 2, want_filters: bool = True, verbose: bool = False):
    """optimize_with_rows (pngloss_image.h:21-25) on an (H, W, 4) uint8 array.  Returns (rgba_out, row_filters|None)."""
    assert rgba.dtype == np.uint8 and rgba.ndim == 3 and rgba.shape[2] == 4
    out = np.ascontiguousarray(rgba).copy()
    h, w = out.shape[:2]
    filt = np.zeros(h, np.uint8) if want_filters else None
    rc = hip_lib().optimize_with_rows(_row_pointers(out), w, h, filt.ctypes.data_as(C.c_void_p) if want_filters else None, verbose, strength, bleed)
    _check(rc, "optimize_with_rows")
    return out, filt


def optimize_with_stride(rgba: np.ndarray, strength: int = 19, bleed: int = 2):
    """optimize_with_stride (pngloss_image.h:17-20): contiguous buffer + stride, row_filters = NULL mode."""
    out = np.ascontiguousarray(rgba).copy()
    h, w = out.shape[:2]
    hip_lib().optimize_with_stride(out.ctypes.data_as(C.c_void_p), w, h, out.strides[0], False, strength, bleed)
    return out


def optimize_for_average_filter(rgba: np.ndarray, strength: int):
    """optimizeForAverageFilter (pngloss_image.h:14-16)."""
    out = np.ascontiguousarray(rgba).copy()
    h, w = out.shape[:2]
    hip_lib().optimizeForAverageFilter(out.ctypes.data_as(C.c_void_p), w, h, strength)
    return out


def optimize_image(packed: np.ndarray, strength: int = 19, bleed: int = 2, want_filters: bool = True):
    """optimize_image (pngloss_image.h:26-29) on an (H, W, bpp) packed uint8 array, bpp 1..4."""
    assert packed.dtype == np.uint8 and packed.ndim == 3 and 1 <= packed.shape[2] <= 4
    out = np.ascontiguousarray(packed).copy()
    h, w, bpp = out.shape
    filt = np.zeros(h, np.uint8) if want_filters else None
    rows = _row_pointers(out)
    img = PnglossImage(C.cast(rows, C.POINTER(C.c_void_p)), w, h, bpp)
    rc = hip_lib().optimize_image(C.byref(img), filt.ctypes.data_as(C.c_void_p) if want_filters else None, False, strength, bleed)
    _check(rc, "optimize_image")
    return out, filt


# ---- device-resident batch extension ------------------------------------------------------------------------

class HipContext:
    """pngloss_hip_ctx wrapper: device-resident batches (pointers come from torch tensors / hipMalloc)."""

    def __init__(self, device: int = -1):
        self._lib = hip_lib()
        self._n = 0
        self._ctx = self._lib.pngloss_hip_create(device)
        if not self._ctx:
            raise RuntimeError("pngloss_hip_create failed: no usable HIP device (there is no CPU fallback)")

    def close(self):
        if self._ctx:
            self._lib.pngloss_hip_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name, value):
        """pngloss_hip_set_option: e.g. ("engine", "seg" | "wg" | "auto"), ("measure", "all" | "visible")"""
        _check(self._lib.pngloss_hip_set_option(self._ctx, name.encode(), value.encode()), "set_option")

    def enqueue(self, images, strength=19, bleed=2, stream=0):
        """images: sequence of (d_rgba_ptr, d_filters_ptr_or_0, width, height). Asynchronous."""
        n = len(images)
        _check(self._lib.pngloss_hip_optimize_batch_async(self._ctx, _image_descs(images), n, strength, bleed, stream or None), "enqueue")
        self._n = n

    def finish(self):
        n = self._n
        res = _array(Result, n)
        _check(self._lib.pngloss_hip_finish(self._ctx, res, n), "finish", partial_ok=True)
        return [_result_dict(r) for r in res[:n]]

    def run(self, images, strength=19, bleed=2, stream=0):
        """pngloss_hip_optimize_batch: the SYNCHRONOUS entry point (enqueue + finish in one call; the library then spares the caller's stream the device-side
        wait for the engine that the asynchronous entry needs)."""
        n = len(images)
        res = _array(Result, n)
        self._n = n
        _check(self._lib.pngloss_hip_optimize_batch(self._ctx, _image_descs(images), n, strength, bleed, stream or None, res), "optimize_batch", partial_ok=True)
        return [_result_dict(r) for r in res[:n]]

    def run_host(self, arrays, strength=19, bleed=2, want_filters=True, inplace=False):
        """pngloss_hip_optimize_batch_host on a list of (H, W, 4) uint8 arrays.  Returns (outs, filters, results).
        inplace: the arrays (C-contiguous uint8) are optimised where they are, like the C call does; otherwise copies are."""
        outs, filts, imgs = _host_images(arrays, want_filters, inplace)
        n = len(outs)
        res = _array(Result, n)
        _check(self._lib.pngloss_hip_optimize_batch_host(self._ctx, imgs, n, strength, bleed, res), "optimize_batch_host", partial_ok=True)
        return outs, filts, [_host_result_dict(r) for r in res[:n]]

    def run_host_emit(self, arrays, strength=19, bleed=2, want_filters=True):
        """pngloss_hip_optimize_batch_host_emit: like run_host, plus per image (color_type, filter_types[H], scanlines[H, W*ch])."""
        outs, filts, imgs = _host_images(arrays, want_filters)
        lines, ids, rows = _scanline_buffers(outs)
        n = len(outs)
        _check(self._lib.pngloss_hip_optimize_batch_host_emit(self._ctx, imgs, n, strength, bleed, _array(Result, n), lines), "optimize_batch_host_emit",
               partial_ok=True)
        return outs, filts, _scanlines_back(lines, ids, rows)

    def run_host_zlib(self, arrays, strength=19, bleed=2, want_filters=True, stream_only=False, want_results=False):
        """pngloss_hip_optimize_batch_host_zlib: like run_host, plus per image (color_type, zlib stream bytes, blocks).
        stream_only: PNGLOSS_HIP_Z_STREAM_ONLY -- the returned pixel arrays are then the unmodified inputs.  want_results: a fourth element, the
        result dicts run_host returns.  With set_option("indexed", "on") a colour type may be 3; palette(index) then has the PLTE / tRNS payloads."""
        outs, filts, imgs = _host_images(arrays, want_filters)
        zs, bufs = _zstreams(self._lib, _shapes(outs), stream_only)
        n = len(outs)
        res = _array(Result, n)
        _check(self._lib.pngloss_hip_optimize_batch_host_zlib(self._ctx, imgs, n, strength, bleed, res, zs), "optimize_batch_host_zlib",
               partial_ok=True)
        out = (outs, filts, _zstreams_back(zs, bufs))
        return out + ([_host_result_dict(r) for r in res[:n]],) if want_results else out

    def run_target(self, images, target, bleed=2, stream=0):
        """pngloss_hip_optimize_batch_target: images as for run(); every image ends up as run() at its chosen strength leaves it.  Synchronous.
        Returns (results, reports): the dicts run() returns and one TargetReport per image.  With a Target2 the call is
        pngloss_hip_optimize_batch_target2 and returns (results, reports, ssim): one Ssim per image, filled when target.min_ssim != 0."""
        n = len(images)
        res, rep = _array(Result, n), _array(TargetReport, n)
        args = (self._ctx, _image_descs(images), n, C.byref(target), bleed, stream or None, res, rep)
        self._n = 0
        if isinstance(target, Target2):
            ssim = _array(Ssim, n)
            _check(self._lib.pngloss_hip_optimize_batch_target2(*args, ssim), "optimize_batch_target2", partial_ok=True)
            return [_result_dict(r) for r in res[:n]], list(rep[:n]), list(ssim[:n])
        _check(self._lib.pngloss_hip_optimize_batch_target(*args), "optimize_batch_target", partial_ok=True)
        return [_result_dict(r) for r in res[:n]], list(rep[:n])

    def run_size(self, images, max_bytes, max_strength=19, bleed=2, stream=0, want_streams=False):
        """pngloss_hip_optimize_batch_size: images as for run(), max_bytes one budget per image; every image ends up as run() at its chosen strength
        leaves it.  Synchronous.  Returns (results, reports, streams): the dicts run() returns, one SizeReport per image and -- with want_streams --
        per image (color_type, zlib stream, blocks), else None."""
        n = len(images)
        res, rep = _array(Result, n), _array(SizeReport, n)
        zs, bufs = _zstreams(self._lib, [(w, h) for (_, _, w, h) in images]) if want_streams else (None, None)
        target = SizeTarget(list(max_bytes), max_strength)
        self._n = 0
        _check(self._lib.pngloss_hip_optimize_batch_size(self._ctx, _image_descs(images), n, C.byref(target), bleed, stream or None, res, zs, rep),
               "optimize_batch_size", partial_ok=True)
        return [_result_dict(r) for r in res[:n]], list(rep[:n]), _zstreams_back(zs, bufs) if want_streams else None

    @property
    def deflate_ms(self):
        return self._lib.pngloss_hip_last_deflate_ms(self._ctx)

    @property
    def engine_ms(self):
        return self._lib.pngloss_hip_last_engine_ms(self._ctx)

    @property
    def total_ms(self):
        return self._lib.pngloss_hip_last_total_ms(self._ctx)

    def png_decode(self, files):
        """pngloss_hip_png_decode_batch_host on a list of PNG file contents (bytes): chunk parsing and inflate on the host (parse_png), the
        inverse filters and the expansion to RGBA8 on the device.  Returns a list of (H, W, 4) uint8 arrays."""
        parsed = [parse_png(f) for f in files]
        outs = _decode_outputs(parsed)
        _check(self._lib.pngloss_hip_png_decode_batch_host(self._ctx, _png_sources(parsed, outs), len(parsed)), "png_decode")
        return outs

    def png_decode_status(self, files):
        """pngloss_hip_png_decode_batch_host_status: like png_decode, but a damaged file only fails itself.  Returns (outs, status list, return code)."""
        parsed = [parse_png(f) for f in files]
        n = len(parsed)
        outs = _decode_outputs(parsed)
        st = _array(C.c_int, n)
        rc = self._lib.pngloss_hip_png_decode_batch_host_status(self._ctx, _png_sources(parsed, outs), n, st)
        return outs, list(st)[:n], rc

    def png_decode_device(self, files, stream=0, pinned=True):
        """pngloss_hip_png_decode_batch_device: the decoded RGBA8 frames STAY on the device.  Returns a list of (device pointer, width, height)
        ready for enqueue()/run() on this context, and the status list.  pinned: the inflated scanlines go up from page-locked memory
        (pngloss_hip_pinned_alloc), as the command line tool does."""
        parsed = [parse_png(f) for f in files]
        n = len(parsed)
        staged, scanlines = [], []
        ptrs, st = _array(C.c_void_p, n), _array(C.c_int, n)
        try:
            for p in parsed:
                sl = p["scanlines"]
                if pinned and len(sl):
                    buf = self._lib.pngloss_hip_pinned_alloc(len(sl))
                    if not buf:
                        raise RuntimeError("pngloss_hip_pinned_alloc failed")
                    staged.append(buf)
                    C.memmove(buf, sl, len(sl))
                    sl = C.cast(buf, C.c_char_p)
                scanlines.append(sl)
            rc = self._lib.pngloss_hip_png_decode_batch_device(self._ctx, _png_sources(parsed, scanlines=scanlines), n, ptrs, st, stream or None)
        finally:
            for b in staged:
                self._lib.pngloss_hip_pinned_free(b)
        if rc not in (0, 25):
            _check(rc, "png_decode_device")
        return _frames(ptrs, parsed), list(st)[:n]

    def png_decode_device_z(self, files, stream=0, zstreams=None):
        """pngloss_hip_png_decode_batch_device_z: the compressed image data goes up, inflate + inverse filters + expansion run on the device, the
        RGBA8 frames stay there.  Returns ([(device pointer, width, height)], status list, return code).  zstreams: replaces the files' own
        streams (tests hand damaged ones in)."""
        parsed = [parse_png(f) for f in files]
        n = len(parsed)
        src = _array(PngZSource, n)
        keep = [zstreams[i] if zstreams is not None else p["zstream"] for i, p in enumerate(parsed)]
        for i, (p, z) in enumerate(zip(parsed, keep)):
            src[i] = PngZSource(z, len(z), p["width"], p["height"], p["ctype"], p["depth"], *_png_chunks(p), interlace=p["interlace"])
        ptrs, st = _array(C.c_void_p, n), _array(C.c_int, n)
        rc = self._lib.pngloss_hip_png_decode_batch_device_z(self._ctx, src, n, ptrs, st, stream or None)
        if rc not in (0, 25):
            _check(rc, "png_decode_device_z")
        return _frames(ptrs, parsed), list(st)[:n], rc

    def engine_info(self, index=0):
        """pngloss_hip_last_engine_info: dict(engine, attempts, restarts, serial_rows, none_dropped) for image `index`."""
        a = (C.c_int32 * 8)()
        _check(self._lib.pngloss_hip_last_engine_info(self._ctx, index, a), "engine_info")
        return dict(engine={3: "segment-parallel", 0: "workgroup-per-image", 4: "row-statistics (strength 0)"}.get(a[0], a[0]), attempts=a[1], restarts=a[2], serial_rows=a[3], none_dropped=a[4], walked_segments=a[5], launch_groups=a[6], stream_wait=a[7])

    def distortion(self, index=0):
        """pngloss_hip_last_distortion: the Distortion of image `index` of the last finished batch, which must have run with
        set_option("distortion", "on") -- otherwise, for an index out of range and while a batch is pending the call fails (pngloss_error 4)."""
        d = Distortion()
        _check(self._lib.pngloss_hip_last_distortion(self._ctx, index, C.byref(d)), "last_distortion")
        return d

    def ssim(self, index=0):
        """pngloss_hip_last_ssim: the Ssim of image `index` of the last finished batch, which must have run with set_option("ssim", "on") --
        otherwise, for an index out of range and while a batch is pending the call fails (pngloss_error 4)."""
        r = Ssim()
        _check(self._lib.pngloss_hip_last_ssim(self._ctx, index, C.byref(r)), "last_ssim")
        return r

    def palette(self, index=0):
        """pngloss_hip_last_palette: the Palette of image `index` of the last finished run_host_zlib, which must have run with
        set_option("indexed", "on") -- otherwise, for an index out of range and while a batch is pending the call fails (pngloss_error 4)."""
        r = Palette()
        _check(self._lib.pngloss_hip_last_palette(self._ctx, index, C.byref(r)), "last_palette")
        return r

    def index_depth(self, index=0):
        """pngloss_hip_last_index_depth: the IndexDepth of image `index` of the last finished run_host_zlib; the rules of palette()."""
        r = IndexDepth()
        _check(self._lib.pngloss_hip_last_index_depth(self._ctx, index, C.byref(r)), "last_index_depth")
        return r

    def quantize(self, images, max_colors=256, rounds=8, stream=0, dither=None, space=None):
        """pngloss_hip_quantize_batch: images as for run() (device-resident RGBA8), quantised in place to at most max_colors colours each.
        Synchronous.  Returns (images, reports): the tuples handed in, whose pixels are the quantised ones now, and one report dict per image
        (QuantReport.as_dict).  dither: None calls that entry point; DITHER_NONE or DITHER_FLOYD_STEINBERG calls pngloss_hip_quantize_batch2
        (include/pngloss_hip_dither.h).  space: None calls what it called without; QUANT_SPACE_RGBA or QUANT_SPACE_VISIBLE calls
        pngloss_hip_quantize_batch3 (include/pngloss_hip_quant_space.h), with dither None as DITHER_NONE."""
        n = len(images)
        rep = _array(QuantReport, n)
        if space is not None:
            params = QuantParams3(max_colors, rounds, dither or DITHER_NONE, space)
            _check(self._lib.pngloss_hip_quantize_batch3(self._ctx, _image_descs(images), n, C.byref(params), rep, stream or None), "quantize_batch3")
        elif dither is None:
            params = QuantParams(max_colors, rounds)
            _check(self._lib.pngloss_hip_quantize_batch(self._ctx, _image_descs(images), n, C.byref(params), rep, stream or None), "quantize_batch")
        else:
            params = QuantParams2(max_colors, rounds, dither)
            _check(self._lib.pngloss_hip_quantize_batch2(self._ctx, _image_descs(images), n, C.byref(params), rep, stream or None), "quantize_batch2")
        return list(images), [r.as_dict() for r in rep[:n]]

    def quantize_target(self, images, target, max_colors=256, rounds=8, dither=DITHER_NONE, stream=0, space=None):
        """pngloss_hip_quantize_batch_target: images as for quantize(), target a QuantTarget.  Every image is quantised in place to the colour count
        the rule of include/pngloss_hip_quant_target.h finds for it, at most max_colors.  Synchronous.  Returns (images, reports): one report dict
        per image (QuantTargetReport.as_dict).  space: None calls that entry point; QUANT_SPACE_RGBA or QUANT_SPACE_VISIBLE calls
        pngloss_hip_quantize_batch_target3 (include/pngloss_hip_quant_space.h)."""
        n = len(images)
        rep = _array(QuantTargetReport, n)
        if space is not None:
            params = QuantParams3(max_colors, rounds, dither, space)
            _check(self._lib.pngloss_hip_quantize_batch_target3(self._ctx, _image_descs(images), n, C.byref(params), C.byref(target), rep, stream or None),
                   "quantize_batch_target3")
        else:
            params = QuantParams2(max_colors, rounds, dither)
            _check(self._lib.pngloss_hip_quantize_batch_target(self._ctx, _image_descs(images), n, C.byref(params), C.byref(target), rep, stream or None),
                   "quantize_batch_target")
        return list(images), [r.as_dict() for r in rep[:n]]

    def compare(self, pairs, stream=0):
        """pngloss_hip_compare_batch: pairs = sequence of (d_a_ptr, d_b_ptr, width, height), device-resident RGBA8; returns one Distortion per pair
        (b against a).  Synchronous."""
        n = len(pairs)
        out = _array(Distortion, n)
        _check(self._lib.pngloss_hip_compare_batch(self._ctx, _image_pairs(pairs), n, out, stream or None), "compare_batch")
        return list(out[:n])

    def compare_ssim(self, pairs, stream=0):
        """pngloss_hip_compare_batch_ssim: pairs as for compare(); returns one Ssim per pair (b against a).  Synchronous."""
        n = len(pairs)
        out = _array(Ssim, n)
        _check(self._lib.pngloss_hip_compare_batch_ssim(self._ctx, _image_pairs(pairs), n, out, stream or None), "compare_batch_ssim")
        return list(out[:n])

    def compare_visible(self, pairs, distortion=True, ssim=True, stream=0):
        """pngloss_hip_compare_batch_visible: pairs as for compare(), measured over visible pixels (alpha-premultiplied channels plus alpha; whatever
        set_option("measure", ...) says).  Returns (list of Distortion or None, list of Ssim or None): None for an output that was not asked for.
        Synchronous."""
        n = len(pairs)
        d = _array(Distortion, n) if distortion else None
        s = _array(Ssim, n) if ssim else None
        _check(self._lib.pngloss_hip_compare_batch_visible(self._ctx, _image_pairs(pairs), n, d, s, stream or None), "compare_batch_visible")
        return (list(d[:n]) if distortion else None), (list(s[:n]) if ssim else None)

    def histogram(self, index=0):
        h = np.zeros(256, np.uint32)
        _check(self._lib.pngloss_hip_last_histogram(self._ctx, index, h.ctypes.data_as(C.c_void_p)), "histogram")
        return h

    def original_tables(self, index=0):
        """pngloss_hip_last_original_tables: (freq, rank) of image `index` of the last finished batch, (5, 256) uint32 each: original_frequency and
        the 8-bit ranks the row engines break ties with.  rank is None for an image the row-statistics engine took (it keeps none)."""
        freq, rank = np.zeros((5, 256), np.uint32), np.zeros((5, 256), np.uint32)
        _check(self._lib.pngloss_hip_last_original_tables(self._ctx, index, freq.ctypes.data_as(C.c_void_p), None), "original_tables")
        a = (C.c_int32 * 8)()
        _check(self._lib.pngloss_hip_last_engine_info(self._ctx, index, a), "engine_info")
        if a[0] == 4:
            return freq, None
        _check(self._lib.pngloss_hip_last_original_tables(self._ctx, index, None, rank.ctypes.data_as(C.c_void_p)), "original_tables")
        return freq, rank


def source_digest():
    """16 hex digits over the text of every kernel / host source of the library (csrc/*.hip, *.h, *.c, sorted by name): what a committed profile was
    taken AT.  tools/gpu_round5.sh stamps every profiles/r05_* file with it and bench.py compares the stamp of the static blocks it quotes with
    the tree it runs from (no .git travels to the GPU box, a content digest does)."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".h", ".c")):
            h.update(name.encode() + b"\0")
            with open(os.path.join(d, name), "rb") as fh:
                h.update(fh.read())
    return h.hexdigest()[:16]


def multi_split(shapes, parts):
    """pngloss_hip_multi_split (the C host's LPT split) for a list of (width, height); returns owner indices.  No GPU needed."""
    n = len(shapes)
    imgs = _array(HostImage, n)
    for i, (w, h) in enumerate(shapes):
        imgs[i] = HostImage(None, None, w, h)
    owner = _array(C.c_int, n)
    hip_lib().pngloss_hip_multi_split(imgs, n, parts, owner)
    return list(owner[:n])


class HipMulti:
    """pngloss_hip_multi wrapper: host-memory batches over every GPU of the node (or the devices named, e.g. "0,0")."""

    def __init__(self, devices=None):
        self._lib = hip_lib()
        self._m = self._lib.pngloss_hip_multi_create(devices.encode() if devices else None)
        if not self._m:
            raise RuntimeError("pngloss_hip_multi_create failed: no usable HIP device (there is no CPU fallback)")

    @property
    def count(self):
        return self._lib.pngloss_hip_multi_count(self._m)

    def close(self):
        if self._m:
            self._lib.pngloss_hip_multi_destroy(self._m)
            self._m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name, value):
        """pngloss_hip_multi_set_option: the option on every context, e.g. ("distortion", "on")"""
        _check(self._lib.pngloss_hip_multi_set_option(self._m, name.encode(), value.encode()), "multi_set_option")

    def distortion(self, index=0):
        """pngloss_hip_multi_last_distortion: the Distortion of arrays[index] of the last run_host, whichever context it went to"""
        d = Distortion()
        _check(self._lib.pngloss_hip_multi_last_distortion(self._m, index, C.byref(d)), "multi_last_distortion")
        return d

    def ssim(self, index=0):
        """pngloss_hip_multi_last_ssim: the Ssim of arrays[index] of the last run_host, whichever context it went to"""
        r = Ssim()
        _check(self._lib.pngloss_hip_multi_last_ssim(self._m, index, C.byref(r)), "multi_last_ssim")
        return r

    def palette(self, index=0):
        """pngloss_hip_multi_last_palette: the Palette of arrays[index] of the last run_host_zlib, whichever context it went to"""
        r = Palette()
        _check(self._lib.pngloss_hip_multi_last_palette(self._m, index, C.byref(r)), "multi_last_palette")
        return r

    def index_depth(self, index=0):
        """pngloss_hip_multi_last_index_depth: the IndexDepth of arrays[index] of the last run_host_zlib, whichever context it went to"""
        r = IndexDepth()
        _check(self._lib.pngloss_hip_multi_last_index_depth(self._m, index, C.byref(r)), "multi_last_index_depth")
        return r

    def quantize_host(self, arrays, max_colors=256, rounds=8, dither=None, space=None):
        """pngloss_hip_multi_quantize_batch_host on a list of (H, W, 4) uint8 arrays.  Returns (outs, reports): the quantised copies and one report
        dict per image (QuantReport.as_dict).  dither: None calls that entry point; DITHER_NONE or DITHER_FLOYD_STEINBERG calls
        pngloss_hip_multi_quantize_batch_host2 (include/pngloss_hip_dither.h).  space: None calls what it called without; QUANT_SPACE_RGBA or
        QUANT_SPACE_VISIBLE calls pngloss_hip_multi_quantize_batch_host3 (include/pngloss_hip_quant_space.h), with dither None as DITHER_NONE."""
        outs, _, imgs = _host_images(arrays, want_filters=False)
        n = len(outs)
        rep = _array(QuantReport, n)
        if space is not None:
            params = QuantParams3(max_colors, rounds, dither or DITHER_NONE, space)
            _check(self._lib.pngloss_hip_multi_quantize_batch_host3(self._m, imgs, n, C.byref(params), rep), "multi_quantize_batch_host3")
        elif dither is None:
            params = QuantParams(max_colors, rounds)
            _check(self._lib.pngloss_hip_multi_quantize_batch_host(self._m, imgs, n, C.byref(params), rep), "multi_quantize_batch_host")
        else:
            params = QuantParams2(max_colors, rounds, dither)
            _check(self._lib.pngloss_hip_multi_quantize_batch_host2(self._m, imgs, n, C.byref(params), rep), "multi_quantize_batch_host2")
        return outs, [r.as_dict() for r in rep[:n]]

    def quantize_host_target(self, arrays, target, max_colors=256, rounds=8, dither=DITHER_NONE, space=None):
        """pngloss_hip_multi_quantize_batch_host_target on a list of (H, W, 4) uint8 arrays, target a QuantTarget.  Returns (outs, reports): the
        quantised copies and one report dict per image (QuantTargetReport.as_dict).  space: None calls that entry point; QUANT_SPACE_RGBA or
        QUANT_SPACE_VISIBLE calls pngloss_hip_multi_quantize_batch_host_target3 (include/pngloss_hip_quant_space.h)."""
        outs, _, imgs = _host_images(arrays, want_filters=False)
        n = len(outs)
        rep = _array(QuantTargetReport, n)
        if space is not None:
            params = QuantParams3(max_colors, rounds, dither, space)
            _check(self._lib.pngloss_hip_multi_quantize_batch_host_target3(self._m, imgs, n, C.byref(params), C.byref(target), rep), "multi_quantize_batch_host_target3")
        else:
            params = QuantParams2(max_colors, rounds, dither)
            _check(self._lib.pngloss_hip_multi_quantize_batch_host_target(self._m, imgs, n, C.byref(params), C.byref(target), rep), "multi_quantize_batch_host_target")
        return outs, [r.as_dict() for r in rep[:n]]

    def run_host(self, arrays, strength=19, bleed=2, want_filters=True):
        outs, filts, imgs = _host_images(arrays, want_filters)
        n = len(outs)
        res = _array(Result, n)
        _check(self._lib.pngloss_hip_multi_optimize_batch_host(self._m, imgs, n, strength, bleed, res, None, None), "multi_optimize_batch_host", partial_ok=True)
        return outs, filts, [_host_result_dict(r) for r in res[:n]]

    def run_host_zlib(self, arrays, strength=19, bleed=2, want_filters=True):
        """pngloss_hip_multi_optimize_batch_host with streams: (outs, filters, results, streams), streams as HipContext.run_host_zlib returns them"""
        outs, filts, imgs = _host_images(arrays, want_filters)
        n = len(outs)
        res = _array(Result, n)
        zs, bufs = _zstreams(self._lib, _shapes(outs))
        _check(self._lib.pngloss_hip_multi_optimize_batch_host(self._m, imgs, n, strength, bleed, res, None, zs), "multi_optimize_batch_host", partial_ok=True)
        return outs, filts, [_host_result_dict(r) for r in res[:n]], _zstreams_back(zs, bufs)

    def run_host_target(self, arrays, target, bleed=2, want_filters=True, emit=None, stream_only=False):
        """pngloss_hip_multi_optimize_batch_host_target on a list of (H, W, 4) uint8 arrays.  emit: None, "scanlines" or "zlib".  Returns
        (outs, filters, results, reports, emitted): emitted is None, or per image what run_host_emit / run_host_zlib return for it.  With a Target2 the
        call is pngloss_hip_multi_optimize_batch_host_target2 and a sixth element follows: one Ssim per image, filled when target.min_ssim != 0."""
        if emit not in (None, "scanlines", "zlib"):
            raise ValueError("emit: None, 'scanlines' or 'zlib'")
        outs, filts, imgs = _host_images(arrays, want_filters)
        n = len(outs)
        lines, ids, rows = _scanline_buffers(outs) if emit == "scanlines" else (None, None, None)
        zs, bufs = _zstreams(self._lib, _shapes(outs), stream_only) if emit == "zlib" else (None, None)
        res, rep = _array(Result, n), _array(TargetReport, n)
        args = (self._m, imgs, n, C.byref(target), bleed, res, lines, zs, rep)
        ssim = _array(Ssim, n) if isinstance(target, Target2) else None
        if ssim is not None:
            _check(self._lib.pngloss_hip_multi_optimize_batch_host_target2(*args, ssim), "multi_optimize_batch_host_target2", partial_ok=True)
        else:
            _check(self._lib.pngloss_hip_multi_optimize_batch_host_target(*args), "multi_optimize_batch_host_target", partial_ok=True)
        emitted = _scanlines_back(lines, ids, rows) if lines is not None else _zstreams_back(zs, bufs) if zs is not None else None
        out = (outs, filts, [_host_result_dict(r) for r in res[:n]], list(rep[:n]), emitted)
        return out + (list(ssim[:n]),) if ssim is not None else out

    def run_host_size(self, arrays, max_bytes, max_strength=19, bleed=2, want_filters=True, emit=None):
        """pngloss_hip_multi_optimize_batch_host_size on a list of (H, W, 4) uint8 arrays.  emit: None, "scanlines", "zlib" or "both".  Returns
        (outs, filters, results, reports, scanlines, streams): the last two None, or per image what run_host_emit / run_host_zlib return for it."""
        if emit not in (None, "scanlines", "zlib", "both"):
            raise ValueError("emit: None, 'scanlines', 'zlib' or 'both'")
        outs, filts, imgs = _host_images(arrays, want_filters)
        n = len(outs)
        lines, ids, rows = _scanline_buffers(outs) if emit in ("scanlines", "both") else (None, None, None)
        zs, bufs = _zstreams(self._lib, _shapes(outs)) if emit in ("zlib", "both") else (None, None)
        res, rep = _array(Result, n), _array(SizeReport, n)
        target = SizeTarget(list(max_bytes), max_strength)
        _check(self._lib.pngloss_hip_multi_optimize_batch_host_size(self._m, imgs, n, C.byref(target), bleed, res, lines, zs, rep),
               "multi_optimize_batch_host_size", partial_ok=True)
        return (outs, filts, [_host_result_dict(r) for r in res[:n]], list(rep[:n]),
                _scanlines_back(lines, ids, rows) if lines is not None else None, _zstreams_back(zs, bufs) if zs is not None else None)
