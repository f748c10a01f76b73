"""sptamd — host side of the MI355X-native wavefront path tracer.

Importing this package loads libspt.so (HIP kernels for gfx950 behind the C
ABI of include/spt.h) and fails loudly when it has not been built.
"""
from . import _lib
from ._lib import (Config, SptError, check, config_from_env, default_adapt_params, default_config, default_denoise_params,
                   default_denoise_var_params, default_params, default_temporal_params, lib, tile_rows)
from .backend import (Accumulator, TemporalAccumulator, temporal_accumulate, HipBackend, Ray3, Scene, TriangleHitInfo, adapt_select, aov_struct, denoise, denoise_var,
                      make_params,
                      queue_stream, read_pfm, envmap_from_latlong, light_table_build, sky_table_build, reference_camera, scene_cache_info, write_pfm)

__all__ = ["_lib", "Config", "SptError", "check", "config_from_env", "default_config", "default_denoise_params",
           "default_denoise_var_params", "default_params", "lib", "tile_rows", "Accumulator", "HipBackend", "Ray3", "Scene",
           "TriangleHitInfo", "adapt_select", "default_adapt_params", "aov_struct", "denoise", "denoise_var", "make_params", "queue_stream", "reference_camera",
           "scene_cache_info", "write_pfm", "read_pfm", "envmap_from_latlong", "light_table_build", "sky_table_build",
           "TemporalAccumulator", "temporal_accumulate", "default_temporal_params"]
