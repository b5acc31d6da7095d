"""ctypes loader for librtus.so (the C ABI in include/rtus.h).

There is NO CPU fallback: if the HIP library is missing or cannot be loaded this module raises,
loudly.  ``oracle/`` is never imported from here.
"""
import ctypes as C
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "librtus.so")
if os.environ.get("RTUS_LIB"):           # experiment builds (scripts/build_variant.sh, interleaved A/B runs): never silently
    LIB_PATH = os.environ["RTUS_LIB"]
    print(f"[rtus] RTUS_LIB is set: loading {LIB_PATH} instead of the in-tree librtus.so", file=sys.stderr)
CSRC = os.path.join(HERE, "csrc")

_lib = None


class RtusError(RuntimeError):
    def __init__(self, status, what):
        self.status = status
        super().__init__(f"{what}: rtus status {status} ({_strerror(status)})")


class Lens(C.Structure):
    """rtus_lens — replaces the reference's module globals c1, c2, l0, h0, d (main_rt.py:449-455)."""
    _fields_ = [("c1", C.c_double), ("c2", C.c_double), ("l0", C.c_double), ("h0", C.c_double),
                ("d", C.c_double)]


class Pipe(C.Structure):
    """rtus_pipe — the pipe of the reference's probe (main_rt.py:451, 466-467) plus its bore."""
    _fields_ = [("r_outer", C.c_double), ("r_inner", C.c_double), ("x_off", C.c_double), ("c3", C.c_double)]


class PipeMedia(C.Structure):
    """rtus_pipe_media — densities and the speeds the lens and the pipe structs do not hold (rtus_leg_amp_pipe)."""
    _fields_ = [("rho_lens", C.c_double), ("ct_lens", C.c_double), ("rho_water", C.c_double), ("rho_wall", C.c_double),
                ("c_l", C.c_double), ("c_t", C.c_double)]


def build(force: bool = False) -> str:
    """Compile librtus.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    args = ["make", "-C", CSRC, "-j4"]
    if force:
        subprocess.run(["make", "-C", CSRC, "clean"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(args, check=True, stdout=subprocess.DEVNULL)
    return LIB_PATH


def _strerror(status):
    try:
        return lib().rtus_strerror(int(status)).decode()
    except Exception:  # pragma: no cover
        return "?"


# Every function of include/rtus.h, once, in the header's order: (name, return type, argument types, since).  `since` is the
# RTUS_VERSION that introduced the entry: 100 stands for every build the loader has met, 101 for "round 4" (older than 107; those
# builds did not yet count a version per feature).  tests/test_abi_and_host.py holds this table to the header, type by type.
# Data pointers are void* (callers pass addresses: numpy's .ctypes.data, torch's .data_ptr()); a typed pointer only where a
# caller hands over a ctypes object.
i, u, ll, sz, dd, vp = C.c_int, C.c_uint, C.c_longlong, C.c_size_t, C.c_double, C.c_void_p
LP, PP, MP = C.POINTER(Lens), C.POINTER(Pipe), C.POINTER(PipeMedia)
i_p, ull_p, vp_p = C.POINTER(C.c_int), C.POINTER(C.c_ulonglong), C.POINTER(C.c_void_p)
PROTOTYPES = (
    ("rtus_strerror", C.c_char_p, [i], 100),
    ("rtus_version", i, [], 100),
    ("rtus_last_hip_error", i, [], 100),
    ("rtus_device_count", i, [i_p], 100),
    ("rtus_release", i, [i], 100),
    ("rtus_selftest", i, [LP, i, ll, ull_p, i], 100),
    # forward trace
    ("rtus_shoot_workspace_bytes", sz, [i], 100),
    ("rtus_shoot_dev", i, [LP, vp, i, vp, vp, i, vp, vp, i, vp, vp, vp, vp, vp, vp, sz, u, vp], 100),
    ("rtus_shoot", i, [LP, vp, i, vp, vp, i, vp, vp, i, vp, vp, vp, vp, vp, u, i], 100),
    # pulse-echo travel times by root-finding
    ("rtus_solve_workspace_bytes", sz, [i, i, i, i], 100),
    ("rtus_solve_path", i, [i, i, i, i, u], 120),
    ("rtus_solve_dev", i, [LP, vp, i, vp, vp, i, vp, i, vp, i, dd, vp, vp, vp, vp, vp, vp, sz, u, vp], 100),
    ("rtus_solve", i, [LP, vp, i, vp, vp, i, vp, i, vp, i, dd, vp, vp, vp, vp, vp, u, i], 100),
    # element matcher
    ("rtus_match_dev", i, [vp, vp, i, i, vp, i, dd, dd, vp, vp, vp, vp], 100),
    ("rtus_match", i, [vp, vp, i, i, vp, i, dd, dd, vp, vp, vp, i], 100),
    ("rtus_ray_hits_dev", i, [vp, i, i, vp, i, dd, dd, vp, vp], 100),
    ("rtus_ray_hits", i, [vp, i, i, vp, i, dd, dd, vp, i], 100),
    # fused sweep
    ("rtus_sweep_workspace_bytes", sz, [i, i, i, i], 100),
    ("rtus_sweep_dev", i, [LP, vp, i, vp, vp, i, vp, vp, i, vp, i, dd, dd, vp, vp, vp, vp, vp, vp, sz, u, vp], 100),
    ("rtus_sweep", i, [LP, vp, i, vp, vp, i, vp, vp, i, vp, i, dd, dd, vp, vp, vp, vp, vp, u, i], 100),
    # travel times through horizontal layers
    ("rtus_tt_layers_dev", i, [vp, vp, i, vp, vp, i, vp, vp, i, vp, vp, vp], 100),
    ("rtus_tt_layers_batch_dev", i, [vp, vp, i, vp, vp, i, ll, vp, vp, i, ll, vp, ll, i, vp], 100),
    ("rtus_tt_layers", i, [vp, vp, i, vp, vp, i, vp, vp, i, vp, vp, i], 100),
    ("rtus_tt_layers_ex_dev", i, [vp, vp, i, vp, vp, i, vp, vp, i, vp, vp, u, vp], 101),
    ("rtus_tt_layers_batch_ex_dev", i, [vp, vp, i, vp, vp, i, ll, vp, vp, i, ll, vp, ll, i, u, vp], 101),
    ("rtus_tt_layers_ex", i, [vp, vp, i, vp, vp, i, vp, vp, i, vp, vp, u, i], 101),
    ("rtus_tt_layers_sort_workspace_bytes", sz, [i], 100),
    ("rtus_tt_layers_sorted_dev", i, [vp, vp, i, vp, vp, i, vp, vp, i, vp, vp, sz, u, vp], 100),
    # travel times through the curved lens surface
    ("rtus_tt_lens_dev", i, [LP, dd, dd, vp, vp, i, vp, vp, i, vp, vp, vp], 100),
    ("rtus_tt_lens", i, [LP, dd, dd, vp, vp, i, vp, vp, i, vp, vp, i], 100),
    ("rtus_tt_lens_f32_dev", i, [LP, dd, dd, vp, vp, i, vp, vp, i, vp, vp, vp], 100),
    ("rtus_tt_lens_f32", i, [LP, dd, dd, vp, vp, i, vp, vp, i, vp, vp, i], 100),
    # row shards of a table, several GPUs
    ("rtus_table_rows_per_block", i, [ll, i, i], 100),
    ("rtus_shard_rows", ll, [ll, i, i, i], 100),
    ("rtus_tt_layers_rows_dev", i, [vp, vp, i, vp, vp, i, ll, ll, vp, vp, i, vp, u, vp], 100),
    ("rtus_tt_lens_rows_dev", i, [LP, dd, dd, vp, vp, i, ll, ll, vp, vp, i, vp, vp, vp], 100),
    ("rtus_tt_lens_f32_rows_dev", i, [LP, dd, dd, vp, vp, i, ll, ll, vp, vp, i, vp, vp, vp], 100),
    ("rtus_tt_lens_stats_dev", i, [LP, dd, dd, vp, vp, i, ll, ll, vp, vp, i, vp, vp, vp], 101),
    ("rtus_tt_lens_f32_stats_dev", i, [LP, dd, dd, vp, vp, i, ll, ll, vp, vp, i, vp, vp, vp], 101),
    ("rtus_tt_layers_multi", i, [vp, vp, i, vp, vp, i, vp, vp, i, vp, i_p, i], 100),
    ("rtus_tt_lens_f32_multi", i, [LP, dd, dd, vp, vp, i, vp, vp, i, vp, i_p, i], 100),
    ("rtus_tt_layers_multi_ex", i, [vp, vp, i, vp, vp, i, vp, vp, i, vp, i_p, i, u], 101),
    ("rtus_tt_layers_multi_ex_dev", i, [vp, vp, i, vp_p, vp_p, i, vp_p, vp_p, i, vp_p, i_p, i, vp_p, i, u], 101),
    ("rtus_tt_layers_multi_dev", i, [vp, vp, i, vp_p, vp_p, i, vp_p, vp_p, i, vp_p, i_p, i, vp_p, i], 100),
    ("rtus_tt_lens_f32_multi_dev", i, [LP, dd, dd, vp_p, vp_p, i, vp_p, vp_p, i, vp_p, i_p, i, vp_p, i], 100),
    # travel times through one measured surface profile
    ("rtus_tt_surface_workspace_bytes", sz, [i], 100),
    ("rtus_tt_surface_dev", i, [dd, dd, vp, i, dd, dd, vp, vp, i, vp, vp, i, vp, vp, vp, sz, vp], 100),
    ("rtus_tt_surface", i, [dd, dd, vp, i, dd, dd, vp, vp, i, vp, vp, i, vp, vp, i], 100),
    # consumers of a travel-time table
    ("rtus_focal_delays_dev", i, [vp, i, i, vp, vp], 100),
    ("rtus_focal_delays", i, [vp, i, i, vp, i], 100),
    ("rtus_tfm_dev", i, [vp, i, i, i, dd, dd, vp, vp, i, vp, vp], 100),
    ("rtus_tfm", i, [vp, i, i, i, dd, dd, vp, vp, i, vp, i], 100),
    # the surface profile from the FMC (adaptive TFM)
    ("rtus_fmc_analytic_dev", i, [vp, i, i, i, i, vp, vp], 100),
    ("rtus_fmc_analytic", i, [vp, i, i, i, i, vp, i], 100),
    ("rtus_surface_find_dev", i, [vp, i, i, dd, dd, vp, vp, dd, dd, dd, i, dd, dd, i, vp, vp, vp, vp], 100),
    ("rtus_surface_find", i, [vp, i, i, dd, dd, vp, vp, dd, dd, dd, i, dd, dd, i, vp, vp, vp, i], 100),
    ("rtus_tfm_analytic_dev", i, [vp, i, i, i, dd, dd, vp, vp, i, vp, vp, vp], 100),
    ("rtus_tfm_analytic", i, [vp, i, i, i, dd, dd, vp, vp, i, vp, vp, i], 100),
    # half-matrix capture
    ("rtus_tfm_hmc_dev", i, [vp, i, i, dd, dd, vp, vp, i, vp, vp], 118),
    ("rtus_tfm_hmc", i, [vp, i, i, dd, dd, vp, vp, i, vp, i], 118),
    ("rtus_tfm_analytic_hmc_dev", i, [vp, i, i, dd, dd, vp, vp, i, vp, vp, vp], 118),
    ("rtus_tfm_analytic_hmc", i, [vp, i, i, dd, dd, vp, vp, i, vp, vp, i], 118),
    # carrier-aware (IQ) interpolation
    ("rtus_tfm_iq_dev", i, [vp, i, i, i, dd, dd, dd, vp, vp, i, vp, vp, vp], 119),
    ("rtus_tfm_iq", i, [vp, i, i, i, dd, dd, dd, vp, vp, i, vp, vp, i], 119),
    ("rtus_tfm_iq_hmc_dev", i, [vp, i, i, dd, dd, dd, vp, vp, i, vp, vp, vp], 119),
    ("rtus_tfm_iq_hmc", i, [vp, i, i, dd, dd, dd, vp, vp, i, vp, vp, i], 119),
    # a stack of frames
    ("rtus_fmc_pack_frames_floats", sz, [i, i, i, i], 121),
    ("rtus_fmc_pack_frames_dev", i, [vp, i, i, i, i, vp, vp], 121),
    ("rtus_tfm_frames_dev", i, [vp, i, i, i, i, dd, dd, vp, vp, i, vp, vp], 121),
    ("rtus_tfm_frames", i, [vp, i, i, i, i, dd, dd, vp, vp, i, vp, i], 121),
    ("rtus_tfm_analytic_frames_dev", i, [vp, i, i, i, i, dd, dd, dd, vp, vp, i, vp, vp, vp], 121),
    ("rtus_tfm_analytic_frames", i, [vp, i, i, i, i, dd, dd, dd, vp, vp, i, vp, vp, i], 121),
    # a stack of int16 frames
    ("rtus_fmc_pack_frames_i16_words", sz, [i, i, i, i], 122),
    ("rtus_fmc_pack_frames_i16_dev", i, [vp, i, i, i, i, vp, vp], 122),
    ("rtus_tfm_frames_i16_dev", i, [vp, i, i, i, i, dd, dd, vp, vp, i, vp, vp], 122),
    ("rtus_tfm_frames_i16", i, [vp, i, i, i, i, dd, dd, vp, vp, i, vp, i], 122),
    ("rtus_tfm_frames_hmc_i16_dev", i, [vp, i, i, i, dd, dd, vp, vp, i, vp, vp], 123),
    ("rtus_tfm_frames_hmc_i16", i, [vp, i, i, i, dd, dd, vp, vp, i, vp, i], 123),
    ("rtus_tfm_frames_hmc_dev", i, [vp, i, i, i, dd, dd, vp, vp, i, vp, vp], 123),
    ("rtus_tfm_frames_hmc", i, [vp, i, i, i, dd, dd, vp, vp, i, vp, i], 123),
    # envelope TFM over a stack of half-matrix frames
    ("rtus_fmc_analytic_i16_dev", i, [vp, i, i, i, i, vp, vp], 125),
    ("rtus_fmc_analytic_i16", i, [vp, i, i, i, i, vp, i], 125),
    ("rtus_fmc_hilbert_pairs_i16_dev", i, [vp, i, i, i, i, vp, vp], 125),
    ("rtus_tfm_envelope_frames_hmc_workspace_bytes", sz, [i, i, i, i, i, dd, i, i], 125),
    ("rtus_tfm_envelope_frames_hmc_i16_dev", i, [vp, i, i, i, i, dd, dd, dd, vp, vp, i, i, vp, vp, vp, sz, vp], 125),
    ("rtus_tfm_envelope_frames_hmc_i16", i, [vp, i, i, i, i, dd, dd, dd, vp, vp, i, i, vp, vp, i], 125),
    ("rtus_tfm_envelope_frames_hmc_dev", i, [vp, i, i, i, i, dd, dd, dd, vp, vp, i, i, vp, vp, vp, sz, vp], 125),
    ("rtus_tfm_envelope_frames_hmc", i, [vp, i, i, i, i, dd, dd, dd, vp, vp, i, i, vp, vp, i], 125),
    # plane-wave imaging
    ("rtus_pw_layers_dev", i, [vp, vp, i, vp, i, dd, dd, dd, vp, vp, i, vp, vp], 107),
    ("rtus_pw_layers", i, [vp, vp, i, vp, i, dd, dd, dd, vp, vp, i, vp, i], 107),
    ("rtus_pw_surface_dev", i, [dd, dd, vp, i, dd, dd, vp, i, dd, dd, dd, vp, vp, i, vp, vp, vp, sz, vp], 107),
    ("rtus_pw_surface", i, [dd, dd, vp, i, dd, dd, vp, i, dd, dd, dd, vp, vp, i, vp, vp, i], 107),
    ("rtus_fmc_synth_tx_dev", i, [vp, i, i, i, dd, vp, i, vp, vp], 107),
    ("rtus_fmc_synth_tx", i, [vp, i, i, i, dd, vp, i, vp, i], 107),
    # backwall skip legs
    ("rtus_tt_surface_skip_dev", i, [dd, dd, vp, i, dd, dd, dd, dd, vp, vp, i, vp, vp, i, vp, vp, vp, vp, sz, vp], 108),
    ("rtus_tt_surface_skip", i, [dd, dd, vp, i, dd, dd, dd, dd, vp, vp, i, vp, vp, i, vp, vp, vp, i], 108),
    # ray amplitudes, weighted TFM
    ("rtus_leg_amp_surface_dev", i, [dd, dd, vp, i, dd, dd, dd, dd, dd, dd, i, i, dd, dd, vp, vp, i, vp, vp, i, vp, vp, vp, vp, sz, vp],
     109),
    ("rtus_leg_amp_surface", i, [dd, dd, vp, i, dd, dd, dd, dd, dd, dd, i, i, dd, dd, vp, vp, i, vp, vp, i, vp, vp, vp, i], 109),
    ("rtus_tfm_weighted_dev", i, [vp, i, i, i, dd, dd, vp, vp, vp, vp, i, vp, vp, vp], 109),
    ("rtus_tfm_weighted", i, [vp, i, i, i, dd, dd, vp, vp, vp, vp, i, vp, vp, i], 109),
    # lens to pipe wall
    ("rtus_tt_pipe_workspace_bytes", sz, [i, i], 110),
    ("rtus_tt_pipe_dev", i, [LP, dd, dd, PP, dd, dd, i, vp, vp, i, vp, vp, i, vp, vp, vp, vp, sz, vp], 110),
    ("rtus_tt_pipe", i, [LP, dd, dd, PP, dd, dd, i, vp, vp, i, vp, vp, i, vp, vp, vp, i], 110),
    # bore-reflected skip legs
    ("rtus_tt_pipe_skip_workspace_bytes", sz, [i, i], 111),
    ("rtus_tt_pipe_skip_dev", i, [LP, dd, dd, PP, dd, dd, dd, i, vp, vp, i, vp, vp, i, vp, vp, vp, vp, vp, sz, vp], 111),
    ("rtus_tt_pipe_skip", i, [LP, dd, dd, PP, dd, dd, dd, i, vp, vp, i, vp, vp, i, vp, vp, vp, vp, i], 111),
    # ray amplitudes into the pipe wall
    ("rtus_leg_amp_pipe_dev", i, [LP, dd, dd, PP, MP, i, i, dd, dd, vp, vp, i, vp, vp, i, vp, vp, vp, vp, vp], 112),
    ("rtus_leg_amp_pipe", i, [LP, dd, dd, PP, MP, i, i, dd, dd, vp, vp, i, vp, vp, i, vp, vp, vp, vp, i], 112),
    # the pipe's geometry from measured echo times
    ("rtus_echo_pick_dev", i, [vp, i, i, i, dd, dd, dd, dd, vp, vp, vp, vp, vp], 113),
    ("rtus_echo_pick", i, [vp, i, i, i, dd, dd, dd, dd, vp, vp, vp, vp, i], 113),
    ("rtus_geom_misfit_dev", i, [vp, i, i, i, vp, vp, vp, vp, vp, vp, vp], 113),
    ("rtus_geom_misfit", i, [vp, i, i, i, vp, vp, vp, vp, vp, vp, i], 113),
    ("rtus_pipe_clearance", dd, [LP, dd, dd, dd], 113),
    # ray-model FMC simulator
    ("rtus_fmc_sim_dev", i, [vp, vp, i, i, i, vp, vp, vp, vp, i, i, i, dd, dd, i, vp, u, vp], 114),
    ("rtus_fmc_sim", i, [vp, vp, i, i, i, vp, vp, vp, vp, i, i, i, dd, dd, i, vp, u, i], 114),
    ("rtus_fmc_sim_echo_dev", i, [vp, vp, i, i, i, vp, i, i, i, dd, dd, i, vp, u, vp], 114),
    ("rtus_fmc_sim_echo", i, [vp, vp, i, i, i, vp, i, i, i, dd, dd, i, vp, u, i], 114),
    # phase-coherence imaging
    ("rtus_tfm_phase_dev", i, [vp, i, i, i, dd, dd, vp, vp, i, vp, vp, vp, vp, vp], 115),
    ("rtus_tfm_phase", i, [vp, i, i, i, dd, dd, vp, vp, i, vp, vp, vp, vp, i], 115),
    # specular echo times of sampled reflectors
    ("rtus_specular_dev", i, [vp, i, vp, i, i, i, vp, vp, vp, vp], 116),
    ("rtus_specular", i, [vp, i, vp, i, i, i, vp, vp, vp, i], 116),
    # skip legs off a sampled backwall
    ("rtus_skip_reflector_dev", i, [vp, i, vp, vp, i, dd, vp, vp, i, vp, vp, vp, vp], 117),
    ("rtus_skip_reflector", i, [vp, i, vp, vp, i, dd, vp, vp, i, vp, vp, vp, i], 117),
    # phase coherence and weighted TFM over a half-matrix capture
    ("rtus_tfm_phase_hmc_dev", i, [vp, i, i, dd, dd, vp, vp, i, vp, vp, vp, vp, vp], 124),
    ("rtus_tfm_phase_hmc", i, [vp, i, i, dd, dd, vp, vp, i, vp, vp, vp, vp, i], 124),
    ("rtus_tfm_weighted_hmc_dev", i, [vp, i, i, dd, dd, vp, vp, vp, vp, i, vp, vp, vp], 124),
    ("rtus_tfm_weighted_hmc", i, [vp, i, i, dd, dd, vp, vp, vp, vp, i, vp, vp, i], 124),
    # matrix arrays: travel times in three dimensions through horizontal layers
    ("rtus_tt_layers3_dev", i, [vp, vp, i, vp, vp, vp, i, vp, vp, vp, i, vp, u, vp], 126),
    ("rtus_tt_layers3", i, [vp, vp, i, vp, vp, vp, i, vp, vp, vp, i, vp, u, i], 126),
    # an anisotropic part: the group slowness as a series in the ray angle
    ("rtus_tt_aniso_surface_dev", i, [dd, dd, vp, i, dd, vp, vp, i, vp, vp, i, vp, vp, i, vp, vp, vp, sz, vp], 127),
    ("rtus_tt_aniso_surface", i, [dd, dd, vp, i, dd, vp, vp, i, vp, vp, i, vp, vp, i, vp, vp, i], 127),
    ("rtus_tt_aniso_direct_dev", i, [vp, vp, i, vp, vp, i, vp, vp, i, vp, vp], 127),
    ("rtus_tt_aniso_direct", i, [vp, vp, i, vp, vp, i, vp, vp, i, vp, i], 127),
)
EXPORTS = tuple(p[0] for p in PROTOTYPES)


def lib():
    """Load librtus.so once; bind every entry of PROTOTYPES."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C ray-tracing-ultrasound_amd/csrc`. There is no CPU fallback.")
    # ONE HIP runtime per process.  The NumPy call surface (api.py, drivers.py) needs no PyTorch and does not import it; but a
    # process may import torch LATER (device.py / dist.py do), and PyTorch's wheel carries its own libamdhip64.so (SONAME
    # libamdhip64.so.7, found by libtorch_hip through RPATH=$ORIGIN under the NAME libamdhip64.so — which glibc does not match
    # against an already loaded /opt/rocm copy).  Two runtimes in one process would hand torch's device pointers and streams to a
    # library bound to the other one.  So when torch is installed its copy of the runtime is loaded first — a dlopen, not an
    # import: librtus.so's NEEDED libamdhip64.so.7 then resolves to it by SONAME, and a later `import torch` finds the same file
    # already mapped.  Without torch the system runtime (/opt/rocm/lib) is used.  RTUS_SYSTEM_HIP=1 skips this.
    if "torch" not in sys.modules and os.environ.get("RTUS_SYSTEM_HIP", "0") != "1":
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is not None and spec.origin:
            hip = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
            if os.path.exists(hip):
                C.CDLL(hip, mode=C.RTLD_GLOBAL)
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, restype, argtypes, since in PROTOTYPES:
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        elif not os.environ.get("RTUS_LIB"):  # an older build loaded through RTUS_LIB for an A/B run keeps this ONE symbol unbound
            raise AttributeError(f"{LIB_PATH} does not export {name} (include/rtus.h, since version {since})")
    _lib = L
    return L


def check(status, what):
    if status != 0:
        raise RtusError(status, what)
