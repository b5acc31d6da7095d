"""rtus — MI355X-native travel-time ray tracer (drop-in for the hot path of
edudscrc/ray-tracing-ultrasound: main_rt.py's shoot_rays + element matcher).

The directory is called ``ray-tracing-ultrasound_amd``; import it as ``import rtus`` (the alias
module at the repo root) or ``importlib.import_module("ray-tracing-ultrasound_amd")``.
"""
from ._lib import EXPORTS, LIB_PATH, Lens, Pipe, PipeMedia, RtusError, build, lib  # noqa: F401
from .api import (ALPHA_MAX, KEYS, Params, configure, match_elements, ray_hits,  # noqa: F401
                  reference_elements, shoot_batch, shoot_rays, travel_time_layers, travel_time_lens, travel_time_surface,
                  fmc_table_layers, solve_travel_times, solve_path, SOLVE_PATHS, focal_delays, tfm_image, sweep_batch, fmc_analytic, measure_surface,
                  adaptive_tfm, tfm_analytic, tfm_phase, pw_delays, pw_travel_time_layers, pw_travel_time_surface, fmc_synth_tx, pwi_image,
                  LEGS, VIEWS, reverse_leg, view_tables, skip_travel_time_layers, skip_travel_time_surface, view_legs_layers,
                  view_legs_surface, tfm_views, leg_amplitudes_surface, view_amplitudes_surface, tfm_weighted,
                  travel_time_pipe, pipe_wall_grid, skip_travel_time_pipe, view_legs_pipe,
                  leg_amplitudes_pipe, view_amplitudes_pipe, pick_echo_times, geom_misfit, pipe_misfit, pipe_clearance, fit_pipe,
                  adaptive_tfm_pipe, gaussian_pulse, simulate_fmc, simulate_echoes, simulate_views, specular_times,
                  backwall_echo_layers, backwall_echo_surface, bore_echo_pipe, fit_reflector, measure_reflector,
                  skip_travel_time_reflector, reflector_mask, skip_travel_time_layers_profile, skip_travel_time_surface_profile,
                  view_legs_layers_profile, view_legs_surface_profile, backwall_profile,
                  hmc_index, hmc_pack, hmc_unpack, hmc_analytic, tfm_hmc, tfm_analytic_hmc, tfm_iq, tfm_iq_hmc, tfm_phase_hmc, tfm_weighted_hmc,
                  centre_frequency, frames_pack, frames_unpack, tfm_frames, frames_pack_i16, frames_unpack_i16,
                  tfm_envelope_frames, fmc_analytic_i16,
                  travel_time_layers_3d, skip_travel_time_layers_3d, view_legs_layers_3d, matrix_array, volume_grid)
from .aniso import (travel_time_surface_aniso, travel_time_aniso, group_slowness_ti, fit_group_slowness,  # noqa: F401
                    elliptical_slowness, eval_group_slowness)

__all__ = ["shoot_rays", "shoot_batch", "sweep_batch", "match_elements", "ray_hits", "travel_time_layers", "travel_time_lens", "travel_time_surface", "fmc_table_layers", "solve_travel_times", "solve_path", "SOLVE_PATHS", "focal_delays", "tfm_image", "fmc_analytic",
           "measure_surface", "adaptive_tfm", "tfm_analytic", "tfm_phase", "pw_delays", "pw_travel_time_layers", "pw_travel_time_surface",
           "fmc_synth_tx", "pwi_image", "LEGS", "VIEWS", "reverse_leg", "view_tables", "skip_travel_time_layers",
           "skip_travel_time_surface", "view_legs_layers", "view_legs_surface", "tfm_views", "leg_amplitudes_surface",
           "view_amplitudes_surface", "tfm_weighted", "travel_time_pipe", "pipe_wall_grid", "skip_travel_time_pipe",
           "view_legs_pipe", "leg_amplitudes_pipe", "view_amplitudes_pipe", "pick_echo_times", "geom_misfit", "pipe_misfit",
           "pipe_clearance", "fit_pipe", "adaptive_tfm_pipe", "gaussian_pulse", "simulate_fmc", "simulate_echoes", "simulate_views", "specular_times",
           "backwall_echo_layers", "backwall_echo_surface", "bore_echo_pipe", "fit_reflector", "measure_reflector",
           "skip_travel_time_reflector", "reflector_mask", "skip_travel_time_layers_profile", "skip_travel_time_surface_profile",
           "view_legs_layers_profile", "view_legs_surface_profile", "backwall_profile", "hmc_index", "hmc_pack",
           "hmc_unpack", "hmc_analytic", "tfm_hmc", "tfm_analytic_hmc", "tfm_iq", "tfm_iq_hmc", "tfm_phase_hmc", "tfm_weighted_hmc", "centre_frequency", "frames_pack",
           "frames_unpack", "tfm_frames", "frames_pack_i16", "frames_unpack_i16", "tfm_envelope_frames",
           "fmc_analytic_i16", "travel_time_layers_3d", "skip_travel_time_layers_3d", "view_legs_layers_3d", "matrix_array",
           "volume_grid", "travel_time_surface_aniso", "travel_time_aniso", "group_slowness_ti", "fit_group_slowness",
           "elliptical_slowness", "eval_group_slowness", "Params",
           "configure", "reference_elements", "ALPHA_MAX", "KEYS", "build", "lib", "RtusError"]
