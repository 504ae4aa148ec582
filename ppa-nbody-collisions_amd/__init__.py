"""Python host side of the MI355X-native N-body + collision stepper.

Thin ctypes mirror of the C ABI in include/nbody.h (library: libnbody_mi355x.so next to this file).  The
class/function names follow the reference's own vocabulary (ConfigData / parseConfigFile /
BodiesData of /root/reference/include/nbodyConfig.h:4-19,22 and src/nbody.cu:47-124) so that tests read
like the reference's main() (src/nbody.cu:373-551).

There is NO fallback: if the shared library is missing the import fails, and every compute call fails with
NbodyError when no gfx950 device is visible.  PyTorch is not needed by this module.
"""
import ctypes
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libnbody_mi355x.so")

F32, F64 = 0, 1
LITERAL, CLEAN = 0, 1
FLAG_RECORD_EVENTS = 1
FLAG_GROUP_EXCHANGE = 2
FLAG_FORCE_COMM = 4
FLAG_TRACK_IDS = 8
TRACER_WALLS = 1
TRACK_PHI = 1
KNN_MAX = 32
SHELLS_MAX = 32
SHELL_MOMENTS_MAX = 8                                           # NBODY_SHELL_MOMENTS_MAX: bins of one library call
SHELL_MOMENTS_WRAPPER_MAX = 32                                  # bins of one shell_moments(): split into calls of <= 8
CELLS_MAX = 1 << 20                                             # NBODY_CELLS_MAX: nx * ny of one call
CELLS_MOMENTS = 1                                               # NBODY_CELLS_MOMENTS
COMM_ID_BYTES = 128
IMAGE_PATH_MAX = 1024

KEYS = ("particleCount", "totalIterations", "save_Image_Every_Xth_Iteration", "timestep", "minRandBodyMass",
        "maxRandBodyMass", "minRadius", "maxRadius", "radiusGrowthRate", "imgWidth", "imgHeight", "fieldWidth",
        "fieldHeight", "imagePath")


class NbodyError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("%s (%d): %s" % (_status_name(status), status, message))
        self.status = status


class ConfigData(ctypes.Structure):
    """struct ConfigData, include/nbodyConfig.h:4-19 (+ `present` bitmask, see include/nbody.h)."""
    _fields_ = [("particleCount", ctypes.c_int), ("totalIterations", ctypes.c_int),
                ("save_Image_Every_Xth_Iteration", ctypes.c_int), ("timestep", ctypes.c_float),
                ("minRandBodyMass", ctypes.c_float), ("maxRandBodyMass", ctypes.c_float),
                ("minRadius", ctypes.c_float), ("maxRadius", ctypes.c_float), ("growthRate", ctypes.c_float),
                ("imgWidth", ctypes.c_int), ("imgHeight", ctypes.c_int), ("fieldWidth", ctypes.c_int),
                ("fieldHeight", ctypes.c_int), ("_imagePath", ctypes.c_char * IMAGE_PATH_MAX),
                ("present", ctypes.c_uint32)]

    @property
    def imagePath(self):
        return self._imagePath.decode("utf-8", "surrogateescape")

    def has(self, key):
        return bool(self.present >> KEYS.index(key) & 1)


class _CtxDesc(ctypes.Structure):
    _fields_ = [("precision", ctypes.c_int), ("semantics", ctypes.c_int), ("capacity", ctypes.c_int),
                ("device", ctypes.c_int), ("rank", ctypes.c_int), ("world", ctypes.c_int),
                ("flags", ctypes.c_uint32), ("event_capacity", ctypes.c_int), ("timestep", ctypes.c_double),
                ("growthRate", ctypes.c_double), ("fieldWidth", ctypes.c_int), ("fieldHeight", ctypes.c_int),
                ("comm_id", ctypes.c_void_p), ("kernel_variant", ctypes.c_int)]


class _BatchParams(ctypes.Structure):
    _fields_ = [("timestep", ctypes.c_double), ("growthRate", ctypes.c_double), ("fieldWidth", ctypes.c_int),
                ("fieldHeight", ctypes.c_int)]


class _BatchDesc(ctypes.Structure):
    _fields_ = [("precision", ctypes.c_int), ("semantics", ctypes.c_int), ("systems", ctypes.c_int),
                ("capacity", ctypes.c_int), ("device", ctypes.c_int), ("flags", ctypes.c_uint32),
                ("event_capacity", ctypes.c_int), ("kernel_variant", ctypes.c_int)]


class Stats(ctypes.Structure):
    _fields_ = [("steps", ctypes.c_int64), ("pairs", ctypes.c_int64), ("force_kernel_ms", ctypes.c_double),
                ("force_kernel_launches", ctypes.c_int64), ("n_bodies", ctypes.c_int), ("n_own", ctypes.c_int),
                ("exchange_ms", ctypes.c_double), ("exchange_launches", ctypes.c_int64),
                ("exchange_bytes", ctypes.c_int64), ("slot_bytes_now", ctypes.c_int64)]


class Diag(ctypes.Structure):
    """struct nbody_diag (include/nbody.h): diagnostics of the resident state, fp64."""
    _fields_ = [("step", ctypes.c_int64), ("n_bodies", ctypes.c_int64), ("coincident_pairs", ctypes.c_int64),
                ("mass", ctypes.c_double), ("momentum", ctypes.c_double * 2), ("center_of_mass", ctypes.c_double * 2),
                ("angular_momentum", ctypes.c_double), ("kinetic", ctypes.c_double), ("potential", ctypes.c_double)]

    def as_dict(self):
        return {"step": self.step, "n_bodies": self.n_bodies, "coincident_pairs": self.coincident_pairs,
                "mass": self.mass, "momentum": (self.momentum[0], self.momentum[1]),
                "center_of_mass": (self.center_of_mass[0], self.center_of_mass[1]),
                "angular_momentum": self.angular_momentum, "kinetic": self.kinetic, "potential": self.potential}


class Field(ctypes.Structure):
    """struct nbody_field (include/nbody.h): acceleration and potential at one point, fp64."""
    _fields_ = [("ax", ctypes.c_double), ("ay", ctypes.c_double), ("phi", ctypes.c_double)]


class Tide(ctypes.Structure):
    """struct nbody_tide (include/nbody.h): the tidal tensor da/dx at one point, fp64."""
    _fields_ = [("txx", ctypes.c_double), ("txy", ctypes.c_double), ("tyy", ctypes.c_double)]


class Neighbor(ctypes.Structure):
    """struct nbody_neighbor (include/nbody.h): the nearest source of one row and the row's overlap count."""
    _fields_ = [("d2", ctypes.c_double), ("index", ctypes.c_int32), ("overlaps", ctypes.c_int32)]


class Rng(ctypes.Structure):
    _fields_ = [("u", ctypes.c_uint64), ("v", ctypes.c_uint64), ("w", ctypes.c_uint64)]


EVENT_DTYPE = np.dtype([("step", np.int32), ("i", np.int32), ("j", np.int32), ("kind", np.int32)])
# struct nbody_lineage: an event in identity space (Stepper.lineage, StepperBatch.lineage)
LINEAGE_DTYPE = np.dtype([("step", np.int32), ("id_i", np.int32), ("id_j", np.int32), ("kind", np.int32)])
# struct nbody_diag as a numpy record (StepperBatch.diagnostics_log)
DIAG_DTYPE = np.dtype([("step", np.int64), ("n_bodies", np.int64), ("coincident_pairs", np.int64), ("mass", np.float64),
                       ("momentum", np.float64, (2,)), ("center_of_mass", np.float64, (2,)),
                       ("angular_momentum", np.float64), ("kinetic", np.float64), ("potential", np.float64)])

# struct nbody_field as a numpy record (Stepper.field, StepperBatch.field)
FIELD_DTYPE = np.dtype([("acc", np.float64, (2,)), ("phi", np.float64)])

# struct nbody_tide as a numpy record; Stepper.tides and StepperBatch.tides return it as (..., 3) float64: txx, txy, tyy
TIDE_DTYPE = np.dtype([("txx", np.float64), ("txy", np.float64), ("tyy", np.float64)])

# struct nbody_neighbor as a numpy record (Stepper.neighbors, StepperBatch.neighbors)
NEIGHBOR_DTYPE = np.dtype([("d2", np.float64), ("index", np.int32), ("overlaps", np.int32)])

# struct nbody_shell_moment (80 bytes) as a numpy record (Stepper.shell_moments, StepperBatch.shell_moments)
SHELL_MOMENT_FIELDS = ("mass", "px", "py", "ke", "mr2", "rad", "ang", "rad2", "ang2")
SHELL_MOMENT_DTYPE = np.dtype([(f, np.float64) for f in SHELL_MOMENT_FIELDS] + [("count", np.int32), ("pad", np.int32)])

# struct nbody_groups_info as a numpy record (Stepper.groups, StepperBatch.groups)
# nbody_grid, nbody_cell and nbody_cells_info (include/nbody.h): the grid, one cell's sums and the summary of cells()
GRID_DTYPE = np.dtype([("x0", np.float64), ("y0", np.float64), ("sx", np.float64), ("sy", np.float64), ("nx", np.int32),
                       ("ny", np.int32)])
CELL_DTYPE = np.dtype([("mass", np.float64), ("px", np.float64), ("py", np.float64), ("k2", np.float64), ("count", np.int32),
                       ("first", np.int32)])
CELLS_INFO_DTYPE = np.dtype([("n", np.int32), ("inside", np.int32), ("outside", np.int32), ("occupied", np.int32),
                             ("largest", np.int32), ("largest_cell", np.int32)])
# nbody_within (24 bytes) and nbody_within_info (32 bytes): one row and the summary of within()
WITHIN_DTYPE = np.dtype([("d2", np.float64), ("index", np.int32), ("count", np.int32), ("overlaps", np.int32), ("cell", np.int32)])
WITHIN_INFO_DTYPE = np.dtype([("total", np.int64), ("n", np.int32), ("rows", np.int32), ("inside", np.int32),
                              ("outside", np.int32), ("largest", np.int32), ("largest_row", np.int32)])
GROUPS_INFO_DTYPE = np.dtype([("n_bodies", np.int32), ("n_groups", np.int32), ("largest", np.int32), ("sweeps", np.int32)])
# nbody_knn_grid_info (24 bytes): the summary of knn(grid=...)
KNN_GRID_INFO_DTYPE = np.dtype([("n", np.int32), ("rows", np.int32), ("inside", np.int32), ("outside", np.int32),
                                ("widened", np.int32), ("rounds", np.int32)])
# nbody_groups_grid_info (24 bytes): the summary of groups(grid=...)
GROUPS_GRID_INFO_DTYPE = np.dtype([("n_bodies", np.int32), ("n_groups", np.int32), ("largest", np.int32), ("sweeps", np.int32),
                                   ("inside", np.int32), ("outside", np.int32)])
# nbody_group_energy_info (24 bytes) and nbody_group_record (80 bytes), include/nbody.h
GROUP_ENERGY_INFO_DTYPE = np.dtype([("n_bodies", np.int32), ("n_groups", np.int32), ("largest", np.int32), ("sweeps", np.int32),
                                    ("coincident", np.int64)])
GROUP_RECORD_DTYPE = np.dtype([("mass", np.float64), ("cx", np.float64), ("cy", np.float64), ("vx", np.float64),
                               ("vy", np.float64), ("kinetic", np.float64), ("potential", np.float64), ("energy", np.float64),
                               ("label", np.int32), ("count", np.int32), ("bound_members", np.int32), ("flags", np.int32)])
GROUP_BOUND = 1                                                 # nbody_group_record.flags bit 0: energy < 0

# struct nbody_pair_info as a numpy record (Stepper.pair_counts, StepperBatch.pair_counts)
PAIR_INFO_DTYPE = np.dtype([("n_bodies", np.int64), ("rows", np.int64), ("pairs", np.int64), ("below", np.int64),
                            ("rest", np.int64)])
# struct nbody_pair_grid_info (56 bytes): nbody_pair_info, then inside and outside (pair_counts(grid=...))
PAIR_GRID_INFO_DTYPE = np.dtype(PAIR_INFO_DTYPE.descr + [("inside", np.int64), ("outside", np.int64)])

# struct nbody_encounter, nbody_encounter_info, nbody_encounter_raw as numpy records (Stepper.encounters,
# StepperBatch.encounters, encounter_finish); ENCOUNTER_DTYPE is what they return: the record without its reserved word
ENCOUNTER_NOW, ENCOUNTER_END = 1, 2
ENCOUNTER_RECORD_DTYPE = np.dtype([("t", np.float64), ("i", np.int32), ("j", np.int32), ("flags", np.uint32), ("reserved", np.uint32)])
ENCOUNTER_DTYPE = np.dtype([("t", np.float64), ("i", np.int32), ("j", np.int32), ("flags", np.uint32)])
ENCOUNTER_INFO_DTYPE = np.dtype([("n_bodies", np.int64), ("pairs", np.int64), ("now", np.int64), ("end", np.int64),
                                 ("missed", np.int64), ("horizon", np.float64)])
ENCOUNTER_RAW_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("flags", np.uint32), ("reserved", np.uint32),
                                ("c", np.float64), ("b", np.float64), ("disc", np.float64)])
# struct nbody_encounter_grid_info (64 bytes): nbody_encounter_info, then inside and outside (encounters(grid=...))
ENCOUNTER_GRID_INFO_DTYPE = np.dtype(ENCOUNTER_INFO_DTYPE.descr + [("inside", np.int64), ("outside", np.int64)])

# struct nbody_binary, nbody_binary_raw, nbody_binary_info as numpy records (Stepper.binaries, StepperBatch.binaries,
# binary_finish); BINARY_DTYPE is what they return: the record without its reserved word
BINARY_OVERLAP, BINARY_APPROACHING = 1, 2
BINARY_RECORD_DTYPE = np.dtype([("a", np.float64), ("ecc", np.float64), ("period", np.float64), ("sep", np.float64),
                                ("i", np.int32), ("j", np.int32), ("flags", np.uint32), ("reserved", np.uint32)])
BINARY_DTYPE = np.dtype([("a", np.float64), ("ecc", np.float64), ("period", np.float64), ("sep", np.float64),
                         ("i", np.int32), ("j", np.int32), ("flags", np.uint32)])
BINARY_RAW_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("flags", np.uint32), ("reserved", np.uint32),
                             ("d2", np.float64), ("v2", np.float64), ("mu", np.float64), ("hz", np.float64)])
BINARY_INFO_DTYPE = np.dtype([("n_bodies", np.int64), ("pairs", np.int64), ("near", np.int64), ("coincident", np.int64),
                              ("overlapping", np.int64), ("approaching", np.int64), ("sep2", np.float64)])
# struct nbody_binary_grid_info (72 bytes): nbody_binary_info, then inside and outside (binaries(grid=...))
BINARY_GRID_INFO_DTYPE = np.dtype(BINARY_INFO_DTYPE.descr + [("inside", np.int64), ("outside", np.int64)])

# struct nbody_tracer / nbody_tracer_info as numpy records (Stepper.set_tracers / tracers, StepperBatch likewise)
TRACER_DTYPE = np.dtype([("pos", np.float64, (2,)), ("vel", np.float64, (2,))])
TRACER_INFO_DTYPE = np.dtype([("steps", np.int64), ("coincident", np.int64), ("count", np.int32), ("flags", np.uint32)])

# struct nbody_track_row, nbody_track_f32 / nbody_track_f64: the planes of the track log (Stepper.tracks, StepperBatch.tracks)
TRACK_ROW_DTYPE = np.dtype([("step", np.int64), ("n_bodies", np.int64)])
TRACK_FIELDS = ("x", "y", "vx", "vy", "m", "r")
TRACK_DTYPE = {F32: np.dtype([(f, np.float32) for f in TRACK_FIELDS]), F64: np.dtype([(f, np.float64) for f in TRACK_FIELDS])}

# every symbol include/nbody.h declares: name -> (restype, argtypes)
_vp, _ip, _i, _f, _d, _sz = (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_float,
                             ctypes.c_double, ctypes.c_size_t)
_pp = ctypes.POINTER(ctypes.c_void_p)
SYMBOLS = {
    "nbody_last_error_string": (ctypes.c_char_p, []),
    "nbody_status_string": (ctypes.c_char_p, [_i]),
    "nbody_abi_version": (_i, []),
    "nbody_block_bytes": (_sz, [_i, _i]),
    "nbody_block_alloc": (_vp, [_i, _i]),
    "nbody_block_free": (None, [_vp]),
    "nbody_block_carve_f32": (_i, [_vp, _i, _pp, _pp, _pp, _pp]),
    "nbody_block_carve_f64": (_i, [_vp, _i, _pp, _pp, _pp, _pp]),
    "nbody_block_compact": (_i, [_vp, _i, _i]),
    "nbody_config_parse": (_i, [ctypes.c_char_p, ctypes.POINTER(ConfigData)]),
    "nbody_config_parse_fd": (_i, [ctypes.c_char_p, ctypes.POINTER(ConfigData), _i]),
    "nbody_config_stock": (None, [ctypes.POINTER(ConfigData)]),
    "nbody_rng_seed": (None, [ctypes.POINTER(Rng), ctypes.c_uint64]),
    "nbody_rng_ival64": (ctypes.c_uint64, [ctypes.POINTER(Rng)]),
    "nbody_rng_fval": (_d, [ctypes.POINTER(Rng)]),
    "nbody_rng_fval_range": (_d, [ctypes.POINTER(Rng), _d, _d]),
    "nbody_init_bodies": (_i, [ctypes.POINTER(ConfigData), _vp, _i]),
    "nbody_init_bodies_seeded": (_i, [ctypes.POINTER(ConfigData), _vp, _i, ctypes.c_uint64]),
    "nbody_ctx_desc_from_config": (None, [ctypes.POINTER(_CtxDesc), ctypes.POINTER(ConfigData), _i]),
    "nbody_ctx_create": (_i, [_pp, ctypes.POINTER(_CtxDesc)]),
    "nbody_ctx_destroy": (_i, [_vp]),
    "nbody_upload": (_i, [_vp, _vp, _i]),
    "nbody_step": (_i, [_vp, _i]),
    "nbody_download": (_i, [_vp, _vp, _ip]),
    "nbody_body_count": (_i, [_vp, _ip]),
    "nbody_sync": (_i, [_vp]),
    "nbody_get_events": (_i, [_vp, _vp, _i, ctypes.POINTER(ctypes.c_int64)]),
    "nbody_clear_events": (_i, [_vp]),
    "nbody_get_ids": (_i, [_vp, _vp, _i, _ip]),
    "nbody_get_lineage": (_i, [_vp, _vp, _i, ctypes.POINTER(ctypes.c_int64)]),
    "nbody_track_reserve": (_i, [_vp, _i, _vp, _i, ctypes.c_uint32]),
    "nbody_track_record": (_i, [_vp]),
    "nbody_track_read": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _ip, _ip]),
    "nbody_get_stats": (_i, [_vp, ctypes.POINTER(Stats)]),
    "nbody_set_kernel_timing": (_i, [_vp, _i]),
    "nbody_force_kernel_name": (ctypes.c_char_p, [_vp]),
    "nbody_render_image": (_i, [_vp, _vp, _i, _i]),
    "nbody_write_pgm": (_i, [ctypes.c_char_p, _vp, _i, _i]),
    "nbody_ctx_info": (_i, [_vp, ctypes.POINTER(_CtxDesc), ctypes.POINTER(ctypes.c_int64)]),
    "nbody_ctx_set_steps": (_i, [_vp, ctypes.c_int64]),
    "nbody_state_save": (_i, [_vp, ctypes.c_char_p]),
    "nbody_group_state_save": (_i, [_pp, _i, ctypes.c_char_p]),
    "nbody_state_load": (_i, [_vp, ctypes.c_char_p]),
    "nbody_state_peek": (_i, [ctypes.c_char_p, _ip, _ip, ctypes.POINTER(ctypes.c_int64)]),
    "nbody_comm_unique_id": (_i, [_vp]),
    "nbody_group_step": (_i, [_pp, _i, _i]),
    "nbody_group_download": (_i, [_pp, _i, _vp, _ip]),
    "nbody_own_range": (_i, [_vp, _ip, _ip]),
    "nbody_partition": (_i, [_i, _i, _i, _ip, _ip]),
    "nbody_ctx_stream": (_vp, [_vp]),
    "nbody_get_diagnostics": (_i, [_vp, ctypes.POINTER(Diag), _vp]),
    "nbody_group_diagnostics": (_i, [_pp, _i, ctypes.POINTER(Diag), _vp]),
    "nbody_get_field": (_i, [_vp, _vp, _i, _vp, _ip, ctypes.POINTER(ctypes.c_int64)]),
    "nbody_get_tides": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _ip, ctypes.POINTER(ctypes.c_int64)]),
    "nbody_get_neighbors": (_i, [_vp, _vp, _i, _vp, _ip]),
    "nbody_get_knn": (_i, [_vp, _vp, _i, _i, _vp, _vp, _ip]),
    "nbody_get_shells": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _ip]),
    "nbody_get_shell_moments": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _ip]),
    "nbody_batch_get_shell_moments": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp]),
    "nbody_get_groups": (_i, [_vp, _d, _d, _vp, _i, _vp]),
    "nbody_get_cells": (_i, [_vp, _vp, ctypes.c_uint32, _vp, _vp, _vp, _vp, _i, _vp]),
    "nbody_batch_get_cells": (_i, [_vp, _vp, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp]),
    "nbody_get_within": (_i, [_vp, _vp, _d, _vp, _i, _vp, _vp, _vp, _i, _vp]),
    "nbody_batch_get_within": (_i, [_vp, _vp, _d, _vp, _i, _vp, _vp, _vp, _i, _vp]),
    "nbody_get_groups_grid": (_i, [_vp, _vp, _d, _d, _vp, _i, _vp]),
    "nbody_batch_get_groups_grid": (_i, [_vp, _vp, _d, _d, _vp, _vp]),
    "nbody_get_knn_grid": (_i, [_vp, _vp, _vp, _i, _i, _d, _d, _vp, _vp, _vp]),
    "nbody_batch_get_knn_grid": (_i, [_vp, _vp, _vp, _i, _i, _d, _d, _vp, _vp, _vp]),
    "nbody_get_pair_counts_grid": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp]),
    "nbody_batch_get_pair_counts_grid": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp]),
    "nbody_get_binaries_grid": (_i, [_vp, _vp, _d, _vp, _i, _vp]),
    "nbody_batch_get_binaries_grid": (_i, [_vp, _vp, _d, _vp, _i, _vp]),
    "nbody_get_group_potential": (_i, [_vp, _d, _d, _vp, _vp, _i, _vp]),
    "nbody_batch_get_group_potential": (_i, [_vp, _d, _d, _vp, _vp, _vp]),
    "nbody_group_catalog": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _ip]),
    "nbody_get_pair_counts": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp]),
    "nbody_get_encounters": (_i, [_vp, _d, _vp, _i, _vp]),
    "nbody_batch_get_encounters": (_i, [_vp, _d, _vp, _i, _vp]),
    "nbody_get_encounters_grid": (_i, [_vp, _vp, _d, _vp, _i, _vp]),
    "nbody_batch_get_encounters_grid": (_i, [_vp, _vp, _d, _vp, _i, _vp]),
    "nbody_encounter_finish": (_i, [_vp, _i, _d, _vp]),
    "nbody_get_binaries": (_i, [_vp, _d, _vp, _i, _vp]),
    "nbody_batch_get_binaries": (_i, [_vp, _d, _vp, _i, _vp]),
    "nbody_binary_finish": (_i, [_vp, _i, _vp]),
    "nbody_tracers_set": (_i, [_vp, _vp, _i, ctypes.c_uint32]),
    "nbody_tracers_get": (_i, [_vp, _vp, _vp, _i, _vp]),
    "nbody_batch_tracers_set": (_i, [_vp, _vp, _i, ctypes.c_uint32]),
    "nbody_batch_tracers_get": (_i, [_vp, _vp, _vp, _vp]),
    "nbody_batch_create": (_i, [_pp, ctypes.POINTER(_BatchDesc), ctypes.POINTER(_BatchParams)]),
    "nbody_batch_destroy": (_i, [_vp]),
    "nbody_batch_upload": (_i, [_vp, _pp, _ip]),
    "nbody_batch_step": (_i, [_vp, _i]),
    "nbody_batch_sync": (_i, [_vp]),
    "nbody_batch_counts": (_i, [_vp, _ip]),
    "nbody_batch_download": (_i, [_vp, _i, _vp, _ip]),
    "nbody_batch_get_events": (_i, [_vp, _i, _vp, _i, ctypes.POINTER(ctypes.c_int64)]),
    "nbody_batch_get_ids": (_i, [_vp, _i, _vp, _i, _ip]),
    "nbody_batch_get_lineage": (_i, [_vp, _i, _vp, _i, ctypes.POINTER(ctypes.c_int64)]),
    "nbody_batch_get_stats": (_i, [_vp, _i, ctypes.POINTER(Stats)]),
    "nbody_batch_kernel_name": (ctypes.c_char_p, [_vp]),
    "nbody_batch_diagnostics": (_i, [_vp, ctypes.POINTER(Diag), _vp]),
    "nbody_batch_get_field": (_i, [_vp, _vp, _i, _vp, ctypes.POINTER(ctypes.c_int64)]),
    "nbody_batch_get_tides": (_i, [_vp, _vp, _vp, _i, _vp, _vp, ctypes.POINTER(ctypes.c_int64)]),
    "nbody_batch_get_neighbors": (_i, [_vp, _vp, _i, _vp]),
    "nbody_batch_get_knn": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "nbody_batch_get_shells": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp]),
    "nbody_batch_get_groups": (_i, [_vp, _d, _d, _vp, _vp]),
    "nbody_batch_get_pair_counts": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp]),
    "nbody_batch_diag_reserve": (_i, [_vp, _i]),
    "nbody_batch_diag_record": (_i, [_vp]),
    "nbody_batch_diag_read": (_i, [_vp, _vp, _i, _ip]),
    "nbody_batch_track_reserve": (_i, [_vp, _i, _vp, _i, ctypes.c_uint32]),
    "nbody_batch_track_record": (_i, [_vp]),
    "nbody_batch_track_read": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _ip, _ip]),
    "nbody_num_blocks": (_i, [_i]),
    "nbody_launch_compute_forces_f32": (_i, [_vp, _vp, _vp, _i, _f, _i, _i, _i, _f, _vp]),
    "nbody_launch_move_bodies_f32": (_i, [_vp, _vp, _vp, _i, _f, _i, _vp]),
    "nbody_launch_workspace_release": (_i, []),
    "nbody_selftest_ieee_f32": (_i, [_i, ctypes.POINTER(ctypes.c_uint64 * 3)]),
    "nbody_selftest_chain_f64": (_i, [_i, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64 * 2)]),
    "nbody_selftest_rcp_ones_f64": (_i, [_i, ctypes.POINTER(ctypes.c_uint64 * 5)]),
    "nbody_selftest_lds_record": (_i, [_i, _i, ctypes.POINTER(ctypes.c_uint64 * 3)]),
    "nbody_debug_ring_probe": (_i, [_vp, ctypes.POINTER(ctypes.c_uint64 * 8)]),
    "nbody_debug_force_only": (_i, [_vp, _i]),
    "nbody_debug_screen_state": (_i, [_vp, _ip, _vp, _i, _ip]),
}


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(or make -C ppa-nbody-collisions_amd/csrc). There is no fallback path." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)     # AttributeError here = header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def _status_name(status):
    return lib.nbody_status_string(status).decode()


def _check(status):
    if status != 0:
        raise NbodyError(status, lib.nbody_last_error_string().decode())


# ---------------------------------------------------------------------------------------------------------
# config / bodies (host side)
# ---------------------------------------------------------------------------------------------------------
def parseConfigFile(path, echo=True):
    """parseConfigFile, include/nbodyConfig.h:22-227. Echoes like the reference unless echo=False.
    Raises NbodyError(NBODY_ERR_IO / NBODY_ERR_PARSE) where the reference calls exit(1)."""
    cfg = ConfigData()
    if echo:
        sys.stdout.flush()
        _check(lib.nbody_config_parse(os.fsencode(path), ctypes.byref(cfg)))
    else:
        _check(lib.nbody_config_parse_fd(os.fsencode(path), ctypes.byref(cfg), -1))
    return cfg


def stock_config(**overrides):
    """The stock nbodyConfig.txt (nbodyConfig.txt:1-14) with keyword overrides of struct fields."""
    cfg = ConfigData()
    lib.nbody_config_stock(ctypes.byref(cfg))
    for k, v in overrides.items():
        if k == "radiusGrowthRate":
            k = "growthRate"
        if not hasattr(cfg, k):
            raise AttributeError(k)
        setattr(cfg, k, v)
    return cfg


def write_config(path, cfg):
    """Writes cfg in the reference's nbodyConfig.txt format (key order of nbodyConfig.txt:1-14)."""
    with open(path, "w") as f:
        f.write("particleCount=%d\ntotalIterations=%d\nsave_Image_Every_Xth_Iteration=%d\n" %
                (cfg.particleCount, cfg.totalIterations, cfg.save_Image_Every_Xth_Iteration))
        f.write("timestep=%.9g\nradiusGrowthRate=%.9g\nminRandBodyMass=%.9g\nmaxRandBodyMass=%.9g\n" %
                (cfg.timestep, cfg.growthRate, cfg.minRandBodyMass, cfg.maxRandBodyMass))
        f.write("minRadius=%.9g\nmaxRadius=%.9g\nimgWidth=%d\nimgHeight=%d\nfieldWidth=%d\nfieldHeight=%d\n" %
                (cfg.minRadius, cfg.maxRadius, cfg.imgWidth, cfg.imgHeight, cfg.fieldWidth, cfg.fieldHeight))
        f.write("imagePath=%s\n" % cfg.imagePath)


class BodiesData:
    """Host body container with the reference's single-allocation layout (struct BodiesData,
    src/nbody.cu:47-124): one flat array [Positions | Velocities | Masses | Radii]."""

    def __init__(self, numBodies, precision=F32, capacity=None):
        self.precision = precision
        self.dtype = np.float64 if precision == F64 else np.float32
        self.capacity = max(int(capacity if capacity is not None else numBodies), int(numBodies), 1)
        self.contiguousData = np.zeros(6 * self.capacity, dtype=self.dtype)
        self.numBodies = int(numBodies)

    @classmethod
    def from_arrays(cls, P, V, M, R, precision=F32):
        b = cls(len(M), precision)
        b.Positions[:] = P
        b.Velocities[:] = V
        b.Masses[:] = M
        b.Radii[:] = R
        return b

    @classmethod
    def from_block(cls, block, numBodies, precision=F32):
        b = cls(numBodies, precision)
        b.contiguousData[:6 * numBodies] = np.asarray(block)[:6 * numBodies]
        return b

    # carving of src/nbody.cu:74-77 for the CURRENT numBodies
    @property
    def Positions(self):
        n = self.numBodies
        return self.contiguousData[:2 * n].reshape(n, 2)

    @property
    def Velocities(self):
        n = self.numBodies
        return self.contiguousData[2 * n:4 * n].reshape(n, 2)

    @property
    def Masses(self):
        n = self.numBodies
        return self.contiguousData[4 * n:5 * n]

    @property
    def Radii(self):
        n = self.numBodies
        return self.contiguousData[5 * n:6 * n]

    @property
    def block(self):
        return self.contiguousData[:6 * self.numBodies]

    @property
    def ptr(self):
        return self.contiguousData.ctypes.data

    def copy(self):
        b = BodiesData(self.numBodies, self.precision, self.capacity)
        b.contiguousData[:] = self.contiguousData
        return b


def init_bodies(cfg, precision=F32, seed=1024):
    """The initial-condition loop of src/nbody.cu:401-416 (x, y, m, r per body; v = 0).  The reference's seed is 1024;
    other seeds give other realisations of the same configuration (nbody_init_bodies_seeded)."""
    b = BodiesData(cfg.particleCount, precision)
    _check(lib.nbody_init_bodies_seeded(ctypes.byref(cfg), b.ptr, precision, seed))
    return b


# ---------------------------------------------------------------------------------------------------------
# device stepper
# ---------------------------------------------------------------------------------------------------------
def saveImageToDisk(filename, img):
    """saveImageToDisk, src/nbody.cu:350-371 (binary PGM)."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    _check(lib.nbody_write_pgm(os.fsencode(filename), img.ctypes.data, img.shape[1], img.shape[0]))


def partition(n, rank, world):
    """(lo, cnt) of rank's own range when n bodies are partitioned over world ranks (nbody_partition)."""
    lo, cnt = ctypes.c_int(0), ctypes.c_int(0)
    _check(lib.nbody_partition(n, rank, world, ctypes.byref(lo), ctypes.byref(cnt)))
    return lo.value, cnt.value


def comm_unique_id():
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    _check(lib.nbody_comm_unique_id(buf))
    return buf.raw


def _ids(call, capacity):
    buf = np.zeros(max(capacity, 1), dtype=np.int32)
    n = ctypes.c_int(0)
    _check(call(buf.ctypes.data, capacity, ctypes.byref(n)))
    return buf[:n.value].copy()


def _lineage(call, cap):
    buf = np.zeros(max(cap, 1), dtype=LINEAGE_DTYPE)
    total = ctypes.c_int64(0)
    _check(call(buf.ctypes.data, cap, ctypes.byref(total)))
    if total.value > cap:
        raise NbodyError(-7, "event log holds %d events, buffer %d" % (total.value, cap))
    return buf[:total.value]


def _diagnostics(call, capacity, potential):
    d = Diag()
    phi = np.zeros(max(capacity, 1), dtype=np.float64) if potential else None
    _check(call(ctypes.byref(d), phi.ctypes.data if potential else None))
    out = d.as_dict()
    if potential:
        out["phi"] = phi[:d.n_bodies].copy()
    return out


def _field_points(points):
    """The probe points of field(): None (the bodies' own positions), or anything np.asarray(..., float64) turns into
    shape (m, 2).  Checked here, before the library is called."""
    if points is None:
        return None
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64))
    if pts.ndim != 2 or pts.shape[1] != 2:
        raise ValueError("points must have shape (m, 2), got %r" % (pts.shape,))
    return pts


def _field(call, points, capacity):
    """nbody_get_field through `call(points, m, out, n_out, coincident)` -> {"acc", "phi", "coincident"}."""
    pts = _field_points(points)
    m = capacity if pts is None else len(pts)
    buf = np.zeros(max(m, 1), dtype=FIELD_DTYPE)
    n, coin = ctypes.c_int(0), ctypes.c_int64(0)
    _check(call(None if pts is None else pts.ctypes.data, m, buf.ctypes.data, ctypes.byref(n), ctypes.byref(coin)))
    return {"acc": np.ascontiguousarray(buf["acc"][:n.value]), "phi": np.ascontiguousarray(buf["phi"][:n.value]),
            "coincident": coin.value}


def _tide_points(points, point_vel, jerk):
    """The rows of tides(): _field_points' points, and their velocities - None (at rest), or shape (m, 2) like the points;
    they need points and jerk=True.  Checked here, before the library is called."""
    pts = _field_points(points)
    if point_vel is None:
        return pts, None
    if pts is None:
        raise ValueError("point_vel needs points: the bodies' own rows have their own velocities")
    if not jerk:
        raise ValueError("point_vel needs jerk=True: the tensor does not depend on a velocity")
    vel = np.ascontiguousarray(np.asarray(point_vel, dtype=np.float64))
    if vel.shape != pts.shape:
        raise ValueError("point_vel must have the points' shape %r, got %r" % (pts.shape, vel.shape))
    return pts, vel


def _tides(call, points, point_vel, jerk, capacity):
    """nbody_get_tides through `call(points, point_vel, m, tide, jerk, n_out, coincident)` -> {"tide", ["jerk",]
    "coincident"}."""
    pts, vel = _tide_points(points, point_vel, jerk)
    m = capacity if pts is None else len(pts)
    tide = np.zeros(max(m, 1), dtype=TIDE_DTYPE)
    jk = np.zeros((max(m, 1), 2), dtype=np.float64) if jerk else None
    n, coin = ctypes.c_int(0), ctypes.c_int64(0)
    _check(call(None if pts is None else pts.ctypes.data, None if vel is None else vel.ctypes.data, m, tide.ctypes.data,
                jk.ctypes.data if jerk else None, ctypes.byref(n), ctypes.byref(coin)))
    out = {"tide": tide[:n.value].view(np.float64).reshape(-1, 3).copy(), "coincident": coin.value}
    if jerk:
        out["jerk"] = np.ascontiguousarray(jk[:n.value])
    return out


def tide_eigen(tide):
    """The eigenvalues of the symmetric 2 x 2 tensors `tide` (..., 3: txx, txy, tyy) -> (lam_max, lam_min), each (...).
    lam = mean +- hypot(half the difference, txy).  Needs no GPU."""
    t = np.asarray(tide, dtype=np.float64)
    if t.shape[-1:] != (3,):
        raise ValueError("tide must have shape (..., 3): txx, txy, tyy, got %r" % (t.shape,))
    mean, half = 0.5 * (t[..., 0] + t[..., 2]), np.hypot(0.5 * (t[..., 0] - t[..., 2]), t[..., 1])
    return mean + half, mean - half


def tidal_radius(tide, mass, G):
    """The tidal (Hill) radius (G m / lam_max)^(1/3) of bodies of mass `mass` in the tides `tide` (..., 3), lam_max the
    larger eigenvalue of tide_eigen; inf where lam_max <= 0 (the tide compresses along every axis).  Needs no GPU."""
    lam = tide_eigen(tide)[0]
    gm = G * np.asarray(mass, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(lam > 0, np.cbrt(gm / np.where(lam > 0, lam, 1.0)), np.inf)


def _tracer_records(pos, vel, systems=None):
    """The tracers of set_tracers() as a TRACER_DTYPE array: pos and vel of shape (m, 2), vel=None meaning zeros; with
    `systems` (a batch) of shape (systems, m, 2), a (m, 2) input being given to every system.  Checked here, before the
    library is called."""
    pos = np.asarray(pos, dtype=np.float64)
    vel = np.zeros_like(pos) if vel is None else np.asarray(vel, dtype=np.float64)
    want = "(m, 2)" if systems is None else "(%d, m, 2) or (m, 2)" % systems
    for name, a in (("pos", pos), ("vel", vel)):
        ok = a.ndim >= 2 and a.shape[-1] == 2 and (a.ndim == 2 or (systems is not None and a.ndim == 3 and a.shape[0] == systems))
        if not ok:
            raise ValueError("%s must have shape %s, got %r" % (name, want, a.shape))
    if systems is not None:
        m = pos.shape[-2]
        pos, vel = (np.broadcast_to(a, (systems, a.shape[-2], 2)) for a in (pos, vel))
        if vel.shape[1] != m:
            raise ValueError("pos has %d tracers per system, vel %d" % (m, vel.shape[1]))
    elif vel.shape != pos.shape:
        raise ValueError("pos has shape %r, vel %r" % (pos.shape, vel.shape))
    rec = np.zeros(pos.shape[:-1], dtype=TRACER_DTYPE)
    rec["pos"], rec["vel"] = pos, vel
    return rec


def _tracer_dict(rec, last, info):
    return {"pos": np.ascontiguousarray(rec["pos"]), "vel": np.ascontiguousarray(rec["vel"]),
            "acc": np.ascontiguousarray(last["acc"]), "phi": np.ascontiguousarray(last["phi"]),
            "steps": info["steps"], "coincident": info["coincident"]}


def _neighbors(call, points, capacity):
    """nbody_get_neighbors through `call(points, m, out, n_out)` -> a NEIGHBOR_DTYPE array, one record per row."""
    pts = _field_points(points)
    m = capacity if pts is None else len(pts)
    buf = np.zeros(max(m, 1), dtype=NEIGHBOR_DTYPE)
    n = ctypes.c_int(0)
    _check(call(None if pts is None else pts.ctypes.data, m, buf.ctypes.data, ctypes.byref(n)))
    return buf[:n.value].copy()


def _knn_buffers(shape):
    """The caller's two arrays of nbody_get_knn, filled with what an empty entry holds."""
    return np.full(shape, np.inf, dtype=np.float64), np.full(shape, -1, dtype=np.int32)


def _groups_dict(label, info):
    return {"label": label, "n_groups": int(info["n_groups"]), "largest": int(info["largest"]), "sweeps": int(info["sweeps"])}


def _groups_grid_dict(label, info, grid):
    d = _groups_dict(label, info)
    d.update(inside=int(info["inside"]), outside=int(info["outside"]), grid=grid[0].copy())
    return d


def _group_potential_dict(label, phi, info):
    d = _groups_dict(label, info)
    d["phi"] = phi
    d["coincident"] = int(info["coincident"])
    return d


def group_catalog(pos, vel, mass, label, phi):
    """nbody_group_catalog, the host half of group_energies(): positions and velocities (n, 2), masses, the labels and the
    in-group potential of group_potential() -> a GROUP_RECORD_DTYPE array, one record per group sorted by label: {mass,
    cx, cy, vx, vy: the centre of mass and its velocity, kinetic: in that frame, potential: 0.5 sum m phi, energy, label,
    count, bound_members: members with 0.5 |v - V|^2 + phi < 0, flags: GROUP_BOUND where energy < 0}.  Every sum is a plain
    fp64 running sum over the group's members in ascending index.  Needs no GPU."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    vel = np.asarray(vel, dtype=np.float64).reshape(-1, 2)
    n = len(pos)
    cols = [np.ascontiguousarray(a, dtype=np.float64) for a in (pos[:, 0], pos[:, 1], vel[:, 0], vel[:, 1], mass, phi)]
    label = np.ascontiguousarray(label, dtype=np.int32)
    if len(vel) != n or label.shape != (n,) or any(c.shape != (n,) for c in cols):
        raise ValueError("group_catalog: pos and vel (n, 2), mass, label and phi (n,) for the same n")
    x, y, vx, vy, m, ph = cols
    count = ctypes.c_int(0)
    _check(lib.nbody_group_catalog(n, x.ctypes.data, y.ctypes.data, vx.ctypes.data, vy.ctypes.data, m.ctypes.data,
                                   label.ctypes.data, ph.ctypes.data, None, 0, ctypes.byref(count)))
    out = np.zeros(max(count.value, 1), dtype=GROUP_RECORD_DTYPE)
    _check(lib.nbody_group_catalog(n, x.ctypes.data, y.ctypes.data, vx.ctypes.data, vy.ctypes.data, m.ctypes.data,
                                   label.ctypes.data, ph.ctypes.data, out.ctypes.data, count.value, ctypes.byref(count)))
    return out[:count.value]


def _group_energies(bodies, g):
    return group_catalog(bodies.Positions, bodies.Velocities, bodies.Masses, g["label"], g["phi"])


def pair_edges2(edges, squared=False):
    """The squared edges pair_counts() sends: `edges` as float64 (B + 1,), each multiplied by itself - one rounding - unless
    they are squared already.  Negative lengths are refused here; everything else (order, NaN, the number of bins) by the
    library."""
    e = np.asarray(edges, dtype=np.float64)
    if e.ndim != 1 or len(e) < 2:
        raise ValueError("edges must have shape (bins + 1,) with bins >= 1, got %r" % (e.shape,))
    if not squared:
        if (e < 0).any():
            raise ValueError("edges are lengths: none may be negative (pass squared=True for squared edges)")
        with np.errstate(over="ignore"):                        # a length above 1.3e154 squares to +inf, a legal top edge
            e = e * e
    return np.ascontiguousarray(e, dtype=np.float64).copy()


def _pair_dict(counts, info, edges2):
    return {"counts": counts, "below": int(info["below"]), "rest": int(info["rest"]), "pairs": int(info["pairs"]),
            "n_bodies": int(info["n_bodies"]), "edges2": edges2}


def _pair_counts(call, systems, edges, points, squared, grid=None):
    """nbody_get_pair_counts through `call(points, m, edges2, bins, counts, info)` -> one dict per system.  With a grid (a
    GRID_DTYPE record) `call` is nbody_get_pair_counts_grid's with the grid bound, and the dicts also have "inside", "outside"
    and "grid"."""
    e2 = pair_edges2(edges, squared)
    pts = _field_points(points)
    bins = len(e2) - 1
    counts = np.zeros((max(systems, 1), bins), dtype=np.uint64)
    info = np.zeros(max(systems, 1), dtype=PAIR_INFO_DTYPE if grid is None else PAIR_GRID_INFO_DTYPE)
    _check(call(None if pts is None else pts.ctypes.data, 0 if pts is None else len(pts), e2.ctypes.data, bins,
                counts.ctypes.data, info.ctypes.data))
    out = [_pair_dict(counts[s].copy(), info[s], e2) for s in range(systems)]
    if grid is not None:
        ins, outs, g = info["inside"].tolist(), info["outside"].tolist(), grid.copy()   # one copy of the grid per call
        for s, d in enumerate(out):
            d.update(inside=ins[s], outside=outs[s], grid=g[0])
    return out


def _shell_buffers(shape):
    """The caller's two arrays of nbody_get_shells, filled with what an empty bin holds."""
    return np.zeros(shape, dtype=np.float64), np.zeros(shape, dtype=np.int32)


def shell_profile(shells):
    """What the radial read-outs are made of, from one result of shells() ({"mass": (rows, B), "count": (rows, B), "edges2":
    (B + 1,)}): {"area": pi * (e2[k+1] - e2[k]) per bin - squared edges give the area of an annulus directly,
    "surface_density": mass / area, "number_density": count / area, "enclosed_mass" and "enclosed_count": cumulative over the
    bins, so they count only what lies at or above the first edge, "half_mass_radius2": per row the squared edge at which
    the enclosed mass first reaches half of the last bin's enclosed mass, NaN for a row without mass}.  Plain numpy in float64
    on the host; needs no GPU and no library call."""
    mass = np.asarray(shells["mass"], dtype=np.float64)
    count = np.asarray(shells["count"])
    e2 = np.asarray(shells["edges2"], dtype=np.float64)
    if mass.ndim != 2 or count.shape != mass.shape or e2.shape != (mass.shape[1] + 1,):
        raise ValueError("shell_profile: mass and count (rows, B) and edges2 (B + 1,) of one shells() result")
    area = np.pi * (e2[1:] - e2[:-1])
    enclosed_mass = np.cumsum(mass, axis=1)
    enclosed_count = np.cumsum(count.astype(np.int64), axis=1)
    total = enclosed_mass[:, -1]
    with np.errstate(invalid="ignore"):
        reached = enclosed_mass >= 0.5 * total[:, None]
    first = np.argmax(reached, axis=1)                          # the first bin that reaches half: its upper edge
    half = np.where(reached.any(axis=1) & (enclosed_count[:, -1] > 0), e2[1:][first], np.nan)
    return {"area": area, "surface_density": mass / area, "number_density": count / area, "enclosed_mass": enclosed_mass,
            "enclosed_count": enclosed_count, "half_mass_radius2": half}


def _shell_moment_rows(points, point_vel):
    """The rows of shell_moments(): _field_points' points, and their velocities - None (at rest), or shape (m, 2) like the
    points; they need points.  Checked here, before the library is called."""
    pts = _field_points(points)
    if point_vel is None:
        return pts, None
    if pts is None:
        raise ValueError("point_vel needs points: the bodies' own rows have their own velocities")
    vel = np.ascontiguousarray(np.asarray(point_vel, dtype=np.float64))
    if vel.shape != pts.shape:
        raise ValueError("point_vel must have the points' shape %r, got %r" % (pts.shape, vel.shape))
    return pts, vel


def _shell_moments(call, shape, e2):
    """nbody_get_shell_moments through `call(edges2, bins, out)` for up to SHELL_MOMENTS_WRAPPER_MAX bins: one library call
    per SHELL_MOMENTS_MAX adjoining bins, each into a buffer of `shape` + (bins of the call,), put side by side.  The bits
    are the same bin for bin: a bin's sums depend on its own two edges only."""
    bins = len(e2) - 1
    if bins > SHELL_MOMENTS_WRAPPER_MAX:
        raise ValueError("shell_moments takes at most %d bins, got %d" % (SHELL_MOMENTS_WRAPPER_MAX, bins))
    out = np.zeros(shape + (bins,), dtype=SHELL_MOMENT_DTYPE)
    for k0 in range(0, bins, SHELL_MOMENTS_MAX):
        k1 = min(k0 + SHELL_MOMENTS_MAX, bins)
        part = np.zeros(shape + (k1 - k0,), dtype=SHELL_MOMENT_DTYPE)
        edges = np.ascontiguousarray(e2[k0:k1 + 1])
        _check(call(edges.ctypes.data, k1 - k0, part.ctypes.data))
        out[..., k0:k1] = part
    return out


def shell_kinematics(result):
    """What the kinematic read-outs are made of, from one result of shell_moments() ({"moments": (..., B) of
    SHELL_MOMENT_DTYPE, ...}) or from such an array itself.  Per (row, bin), float64, with u the sources' velocity relative to
    the row and d their offset from it:
      "mean_velocity" (..., B, 2): (px, py) / mass, the mass-weighted mean of u;
      "sigma2": ke / mass - |mean_velocity|^2, the velocity dispersion about that mean (both components together);
      "mean_r2": mr2 / mass, the mass-weighted mean squared distance;
      "expansion_rate": rad / mr2 and "rotation_rate": ang / mr2 - H and Omega of the mass-weighted least-squares fit of
        u = H d + Omega z x d to the bin (the normal equations are sum m d.u = H sum m d2 and sum m d x u = Omega sum m d2);
      "vr2": rad2 / mr2 and "vt2": ang2 / mr2, the r^2-weighted mean squares of the radial and the tangential velocity;
      "anisotropy": 1 - (vt2 - rotation_rate^2 mean_r2) / (vr2 - expansion_rate^2 mean_r2): the fitted flow's share H^2 r^2 or
        Omega^2 r^2 is taken off each mean square with r^2 = mean_r2, which is exact for a thin bin and an estimate for a
        wide one (the r^2-weighted mean of r^2 is sum m d2^2 / sum m d2, which the sums do not hold).  0 for isotropic
        residuals, towards 1 for radial ones, negative for tangential ones.  Where the residual radial motion is nothing
        but rounding - a pure rotation, a pure expansion, a bin at rest - the denominator is noise or 0 and the value is
        meaningless or NaN.
    Every entry of an empty bin (count == 0) is NaN.  Plain numpy on the host; needs no GPU and no library call."""
    mom = result["moments"] if isinstance(result, dict) else result
    mom = np.asarray(mom)
    if mom.dtype != SHELL_MOMENT_DTYPE:
        raise ValueError("shell_kinematics: the \"moments\" of one shell_moments() result, got dtype %r" % (mom.dtype,))
    empty = mom["count"] == 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        mass, mr2 = mom["mass"], mom["mr2"]
        mean = np.stack([mom["px"] / mass, mom["py"] / mass], axis=-1)
        sigma2 = mom["ke"] / mass - ((mean[..., 0] * mean[..., 0]) + (mean[..., 1] * mean[..., 1]))
        mean_r2 = mr2 / mass
        H, W = mom["rad"] / mr2, mom["ang"] / mr2
        vr2, vt2 = mom["rad2"] / mr2, mom["ang2"] / mr2
        beta = 1.0 - (vt2 - (W * W) * mean_r2) / (vr2 - (H * H) * mean_r2)
    out = {"mean_velocity": mean, "sigma2": sigma2, "mean_r2": mean_r2, "expansion_rate": H, "rotation_rate": W, "vr2": vr2,
           "vt2": vt2, "anisotropy": beta}
    for name, a in out.items():
        a[empty] = np.nan
    return out


def make_grid(nx, ny=None, bounds=None):
    """The nbody_grid of cells(): nx x ny cells (ny=None: nx) over bounds = (x0, x1, y0, y1), the half-open rectangle
    [x0, x1) x [y0, y1) -> a GRID_DTYPE record with sx = nx / (x1 - x0) and sy = ny / (y1 - y0), computed once in fp64: the
    definition of the cell sums uses those doubles as they are.  A GRID_DTYPE record passes through unchanged."""
    if isinstance(nx, np.ndarray) or isinstance(nx, np.void):
        g = np.zeros(1, dtype=GRID_DTYPE)
        g[0] = np.asarray(nx, dtype=GRID_DTYPE).reshape(-1)[0]
        return g
    if bounds is None:
        raise ValueError("make_grid needs bounds = (x0, x1, y0, y1)")
    x0, x1, y0, y1 = (np.float64(v) for v in bounds)
    nx = int(nx)
    ny = nx if ny is None else int(ny)
    g = np.zeros(1, dtype=GRID_DTYPE)
    with np.errstate(divide="ignore", invalid="ignore"):
        g[0] = (x0, y0, np.float64(nx) / (x1 - x0), np.float64(ny) / (y1 - y0), nx, ny)
    return g


def _field_bounds(field):
    """The default bounds of cells(): the field, where nbody_init_bodies places bodies."""
    if field is None:
        raise ValueError("cells() needs bounds: this handle was created without field sizes")
    w, h = field
    return (-float(w), float(w), -float(h), float(h))


def _cells_grid(grid_or_nx, ny, bounds, field):
    if isinstance(grid_or_nx, (np.ndarray, np.void)):
        return make_grid(grid_or_nx)
    return make_grid(grid_or_nx, ny, _field_bounds(field) if bounds is None else bounds)


def _cells(call, systems, capacity, grid, moments, lists):
    """nbody_get_cells through `call(grid, flags, cells, cell_of, start, order, info)` for `systems` systems (None: a
    context) -> the raw arrays (cells (S, ny, nx), cell_of (S, capacity), start (S, cells + 1), order (S, capacity), info (S,));
    the lists None without `lists`."""
    S = 1 if systems is None else systems
    nx, ny = int(grid["nx"][0]), int(grid["ny"][0])
    room = max(nx, 0) * max(ny, 0) if 0 < nx * ny <= CELLS_MAX else 1
    cells = np.zeros((max(S, 1), room), dtype=CELL_DTYPE)
    info = np.zeros(max(S, 1), dtype=CELLS_INFO_DTYPE)
    cell_of = start = order = None
    if lists:
        cell_of = np.full((max(S, 1), max(capacity, 1)), -1, dtype=np.int32)
        order = np.full((max(S, 1), max(capacity, 1)), -1, dtype=np.int32)
        start = np.zeros((max(S, 1), room + 1), dtype=np.int32)
    _check(call(grid.ctypes.data, CELLS_MOMENTS if moments else 0, cells.ctypes.data,
                cell_of.ctypes.data if lists else None, start.ctypes.data if lists else None,
                order.ctypes.data if lists else None, info.ctypes.data))
    return cells.reshape(max(S, 1), ny, nx), cell_of, start, order, info


def _cells_dict(cells, cell_of, start, order, info, grid):
    out = {"cells": cells, "grid": grid[0].copy(), "info": {k: int(info[k]) for k in CELLS_INFO_DTYPE.names}}
    if cell_of is not None:
        out["cell_of"] = cell_of[:out["info"]["n"]].copy()
        out["start"] = start.copy()
        out["order"] = order[:out["info"]["inside"]].copy()
    return out


def within_grid(field, radius, squared=False, most=1024):
    """The default grid of within(): the field's bounds [-w, w) x [-h, h) (field = (w, h)) in cells no smaller than `radius`
    per side (a squared length with squared=True) and at most `most` per axis - the grid on which a row's window is 3 x 3
    cells.  radius 0 gives `most` cells per axis, +inf one."""
    w, h = (float(v) for v in field)
    r = float(radius)
    r = float(np.sqrt(np.float64(r))) if squared else r
    most = max(int(most), 1)

    def along(extent):
        if not r > 0.0:
            return most
        return int(min(max(np.floor(extent / r), 1.0), float(most)))
    return make_grid(along(2.0 * w), along(2.0 * h), (-w, w, -h, h))


def groups_grid(field, link, radius_scale, r_typical, most=1024):
    """The grid to hand groups(grid=...): within_grid(field, radius_scale * 2 * r_typical + link, most=most), the field's
    bounds in cells no smaller than the reach of a TYPICAL body - the median radius of the state, say - and at most `most`
    per axis.  The cell side should match the typical reach, not the largest: a row's window is as wide as its OWN radius
    asks, so a body ten times the typical size walks more cells itself and widens nobody else's window, while cells sized
    to the largest body would make every small body test all of a large cell's members."""
    return within_grid(field, float(radius_scale) * 2.0 * float(r_typical) + float(link), most=most)


def encounters_grid(field, horizon, r_typical, v_typical, most=1024):
    """The grid to hand encounters(grid=...): within_grid(field, 2 * (r_typical + horizon * v_typical), most=most), the
    field's bounds in cells no smaller than twice the reach of a TYPICAL body within the horizon - the median radius and the
    median of |vx| + |vy| of the state, say - and at most `most` per axis: the grid on which a typical row's window is 3 x 3
    cells.  A row's window is as wide as its OWN reach asks, so one fast or large body walks more cells itself and widens
    nobody else's window."""
    return within_grid(field, 2.0 * (float(r_typical) + float(horizon) * float(v_typical)), most=most)


def knn_grid(field, k, n, most=1024):
    """The grid to hand knn(grid=...): the field's bounds [-w, w) x [-h, h) (field = (w, h)) in square-ish cells that hold
    about k of n bodies each at uniform density - side sqrt(area * k / n) - and at most `most` per axis: the grid on which
    a row's first window of 3 x 3 cells holds about 9 k candidates."""
    w, h = (float(v) for v in field)
    k, n, most = max(int(k), 1), max(int(n), 1), max(int(most), 1)
    side = float(np.sqrt(np.float64(4.0 * w * h) * k / n))

    def along(extent):
        if not side > 0.0:
            return most
        return int(min(max(np.floor(extent / side), 1.0), float(most)))
    return make_grid(along(2.0 * w), along(2.0 * h), (-w, w, -h, h))


def _knn_grid(call, systems, per_own, k, points, grid, h0, max_radius, squared):
    """nbody_get_knn_grid through `call(grid, points, m, k, h0, h2_max, d2, index, info)` for `systems` systems (None: a
    context) -> (d2 (S, per, k), index (S, per, k), info (S,), whether the rows are points).  h0=None: the larger cell side;
    max_radius=None: +inf, otherwise squared with one float64 multiply unless `squared`."""
    pts = _field_points(points)
    k = int(k)
    S = 1 if systems is None else max(systems, 1)
    per = per_own if pts is None else len(pts)
    if h0 is None:
        h0 = max(1.0 / float(grid["sx"][0]), 1.0 / float(grid["sy"][0]))
    r = np.inf if max_radius is None else float(max_radius)
    h2_max = r if squared or max_radius is None else r * r
    d2, index = _knn_buffers((S, max(per, 1), max(k, 1)))
    info = np.zeros(S, dtype=KNN_GRID_INFO_DTYPE)
    _check(call(grid.ctypes.data, None if pts is None else pts.ctypes.data, per, k, float(h0), h2_max, d2.ctypes.data,
                index.ctypes.data, info.ctypes.data))
    return d2, index, info, pts is not None


def _knn_grid_dict(d2, index, info, grid):
    rows = int(info["rows"])
    return {"d2": d2[:rows].copy(), "index": index[:rows].copy(), "info": {f: int(info[f]) for f in KNN_GRID_INFO_DTYPE.names},
            "grid": grid[0].copy()}


def _within(call, systems, per_own, radius, points, grid, squared, lists):
    """nbody_get_within through `call(grid, h2, points, m, out, start, list, cap, info)` for `systems` systems (None: a
    context) -> one dict per system: {"rows": WITHIN_DTYPE (rows,), "info", "grid"} and with `lists` "start": int64
    (rows + 1,) and "list": int32 (total,).  radius is squared with one float64 multiply unless `squared`.  On
    NBODY_ERR_CAPACITY the call is repeated once with the largest info.total."""
    h = float(radius)
    h2 = h if squared else h * h
    pts = _field_points(points)
    S = 1 if systems is None else max(systems, 1)
    per = per_own if pts is None else len(pts)
    rows = np.empty((S, max(per, 1)), dtype=WITHIN_DTYPE)       # only what the library has filled is handed out
    info = np.zeros(S, dtype=WITHIN_INFO_DTYPE)
    start = np.empty((S, per + 1), dtype=np.int64) if lists else None
    cap = max(16 * per, 64) if lists else 0                     # the first guess of the room
    lst = np.empty((S, cap), dtype=np.int32) if lists else None

    def once():
        return call(grid.ctypes.data, h2, None if pts is None else pts.ctypes.data, per, rows.ctypes.data,
                    start.ctypes.data if lists else None, lst.ctypes.data if lists else None, cap, info.ctypes.data)
    status = once()
    if status == -7 and lists and int(info["total"].max()) > cap:   # NBODY_ERR_CAPACITY: info is complete
        cap = int(info["total"].max())
        lst = np.empty((S, cap), dtype=np.int32)
        status = once()
    _check(status)
    out = []
    for s in range(S if systems is None else systems):
        k = int(info["rows"][s])
        d = {"rows": rows[s, :k], "info": {f: int(info[f][s]) for f in WITHIN_INFO_DTYPE.names}, "grid": grid[0].copy()}
        if lists:
            d["start"] = start[s, :k + 1]
            d["list"] = lst[s, :int(info["total"][s])]
        out.append(d)
    return out


def cell_maps(result):
    """What the sums of cells() are for, on the host in numpy, from its result (a dict with "cells" and "grid", one system):
    {"area": of one cell, "surface_density": mass / area, "mean_velocity": (ny, nx, 2) p / mass, "dispersion": the velocity
    dispersion k2 / mass - |p|^2 / mass^2 (both NaN where a cell is empty; they need moments=True), "cic_mean", "cic_variance",
    "cic_ratio": the mean, the population variance and variance / mean of the counts over the cells - 1 for a Poisson
    process, above for a clustered one."""
    cells, g = np.asarray(result["cells"]), result["grid"]
    if cells.dtype != CELL_DTYPE or cells.ndim != 2:
        raise ValueError("cell_maps takes the result of one system: a CELL_DTYPE array (ny, nx)")
    area = (1.0 / float(g["sx"])) * (1.0 / float(g["sy"]))
    mass, count = cells["mass"], cells["count"]
    with np.errstate(divide="ignore", invalid="ignore"):
        vel = np.stack([cells["px"] / mass, cells["py"] / mass], axis=-1)
        disp = cells["k2"] / mass - (cells["px"] * cells["px"] + cells["py"] * cells["py"]) / (mass * mass)
    vel[count == 0] = np.nan
    disp = np.where(count == 0, np.nan, disp)
    mean = float(count.mean())
    var = float(count.astype(np.float64).var())
    return {"area": area, "surface_density": mass / area, "mean_velocity": vel, "dispersion": disp, "cic_mean": mean,
            "cic_variance": var, "cic_ratio": var / mean if mean > 0 else float("nan")}


def _encounter_list(rec):
    out = np.zeros(len(rec), dtype=ENCOUNTER_DTYPE)
    for f in ENCOUNTER_DTYPE.names:
        out[f] = rec[f]
    return out


def _encounter_info(info):
    d = {k: int(info[k]) for k in ("n_bodies", "pairs", "now", "end", "missed")}
    d["horizon"] = float(info["horizon"])
    return d


def _encounters(call, systems, horizon, cap, grid=None):
    """nbody_get_encounters through `call(horizon, out, cap, info)` -> one (ENCOUNTER_DTYPE array, info dict) per system.  On
    NBODY_ERR_CAPACITY the call is repeated once with the largest info.pairs.  With a grid (a GRID_DTYPE record) `call` is
    nbody_get_encounters_grid's with the grid bound, and the info dicts also have "inside", "outside" and "grid"."""
    S = max(systems, 1)
    info = np.zeros(S, dtype=ENCOUNTER_INFO_DTYPE if grid is None else ENCOUNTER_GRID_INFO_DTYPE)
    cap = max(int(cap), 0)
    buf = np.zeros((S, max(cap, 1)), dtype=ENCOUNTER_RECORD_DTYPE)
    status = call(horizon, buf.ctypes.data, cap, info.ctypes.data)
    if status == -7:                                            # NBODY_ERR_CAPACITY: info is complete
        cap = int(info["pairs"].max())
        buf = np.zeros((S, max(cap, 1)), dtype=ENCOUNTER_RECORD_DTYPE)
        status = call(horizon, buf.ctypes.data, cap, info.ctypes.data)
    _check(status)
    out = [(_encounter_list(buf[s, :int(info["pairs"][s])]), _encounter_info(info[s])) for s in range(systems)]
    if grid is not None:
        ins, outs, g = info["inside"].tolist(), info["outside"].tolist(), grid.copy()   # one copy of the grid per call
        for s, (_, d) in enumerate(out):
            d.update(inside=ins[s], outside=outs[s], grid=g[0])
    return out


def encounter_finish(raw, horizon):
    """nbody_encounter_finish, the host half of encounters(): ENCOUNTER_RAW_DTYPE records {i, j, flags, c, b, disc} of swept
    pairs -> the ENCOUNTER_DTYPE list {t, i, j, flags} sorted by (t, i, j).  Needs no GPU."""
    raw = np.ascontiguousarray(raw, dtype=ENCOUNTER_RAW_DTYPE)
    out = np.zeros(max(len(raw), 1), dtype=ENCOUNTER_RECORD_DTYPE)
    _check(lib.nbody_encounter_finish(raw.ctypes.data, len(raw), float(horizon), out.ctypes.data))
    return _encounter_list(out[:len(raw)])


def first_contacts(enc, n):
    """Per body of n, from an encounters() list: {"t": the earliest contact time (+inf: none), "partner": the other body of
    that encounter (-1; ties in t go to the earlier record of the list), "count": the encounters the body is part of}."""
    t = np.full(n, np.inf)
    partner = np.full(n, -1, dtype=np.int32)
    m = len(enc)
    body = np.concatenate([enc["i"], enc["j"]]).astype(np.int64)
    other = np.concatenate([enc["j"], enc["i"]])
    rec = np.concatenate([np.arange(m), np.arange(m)])
    order = np.argsort(rec, kind="stable")                      # the list is sorted by t: a body's first record is its earliest
    body, other, rec = body[order], other[order], rec[order]
    who, first = np.unique(body, return_index=True)
    t[who] = enc["t"][rec[first]]
    partner[who] = other[first]
    count = np.bincount(body, minlength=n).astype(np.int64)
    return {"t": t, "partner": partner, "count": count}


def _binary_list(rec):
    out = np.zeros(len(rec), dtype=BINARY_DTYPE)
    for f in BINARY_DTYPE.names:
        out[f] = rec[f]
    return out


def _binary_info(info):
    d = {k: int(info[k]) for k in ("n_bodies", "pairs", "near", "coincident", "overlapping", "approaching")}
    d["sep2"] = float(info["sep2"])
    return d


def _binaries(call, systems, max_sep, squared, cap, grid=None):
    """nbody_get_binaries through `call(sep2, out, cap, info)` -> one (BINARY_DTYPE array, info dict) per system.  max_sep is
    squared with one float64 multiply unless `squared`.  On NBODY_ERR_CAPACITY the call is repeated once with the largest
    info.pairs.  With a grid (a GRID_DTYPE record) `call` is nbody_get_binaries_grid's with the grid bound, and the info
    dicts also have "inside", "outside" and "grid"."""
    sep = float(max_sep)
    sep2 = sep if squared else sep * sep
    S = max(systems, 1)
    info = np.zeros(S, dtype=BINARY_INFO_DTYPE if grid is None else BINARY_GRID_INFO_DTYPE)
    cap = max(int(cap), 0)
    buf = np.zeros((S, max(cap, 1)), dtype=BINARY_RECORD_DTYPE)
    status = call(sep2, buf.ctypes.data, cap, info.ctypes.data)
    if status == -7:                                            # NBODY_ERR_CAPACITY: info is complete
        cap = int(info["pairs"].max())
        buf = np.zeros((S, max(cap, 1)), dtype=BINARY_RECORD_DTYPE)
        status = call(sep2, buf.ctypes.data, cap, info.ctypes.data)
    _check(status)
    out = [(_binary_list(buf[s, :int(info["pairs"][s])]), _binary_info(info[s])) for s in range(systems)]
    if grid is not None:
        ins, outs, g = info["inside"].tolist(), info["outside"].tolist(), grid.copy()   # one copy of the grid per call
        for s, (_, d) in enumerate(out):
            d.update(inside=ins[s], outside=outs[s], grid=g[0])
    return out


def binary_finish(raw):
    """nbody_binary_finish, the host half of binaries(): BINARY_RAW_DTYPE records {i, j, flags, d2, v2, mu, hz} of bound pairs
    -> the BINARY_DTYPE list {a, ecc, period, sep, i, j, flags} sorted by (i, j).  Needs no GPU."""
    raw = np.ascontiguousarray(raw, dtype=BINARY_RAW_DTYPE)
    out = np.zeros(max(len(raw), 1), dtype=BINARY_RECORD_DTYPE)
    _check(lib.nbody_binary_finish(raw.ctypes.data, len(raw), out.ctypes.data))
    return _binary_list(out[:len(raw)])


def _reserve_tracks(call, samples, ids, potential):
    """-> (samples, has_phi): what tracks() needs to size its buffers."""
    k = 0 if ids is None else len(ids)
    sel = np.zeros(max(k, 1), dtype=np.int32)                   # an empty selection is still a pointer: refused by the library
    sel[:k] = [] if ids is None else ids
    _check(call(samples, None if ids is None else sel.ctypes.data, k, TRACK_PHI if potential else 0))
    return samples, bool(potential)


def _tracks(call, reserved, systems, precision):
    """Reads the track log: a dict of numpy arrays, (samples, systems, columns) (rows: (samples, systems))."""
    cap, has_phi = reserved
    n, cols = ctypes.c_int(0), ctypes.c_int(0)
    _check(call(None, None, None, None, 0, ctypes.byref(n), ctypes.byref(cols)))   # how much there is
    take, k = min(n.value, cap), cols.value
    rows = np.zeros((take, systems), dtype=TRACK_ROW_DTYPE)
    rec = np.zeros((take, systems, k), dtype=TRACK_DTYPE[precision])
    index = np.zeros((take, systems, k), dtype=np.int32)
    phi = np.zeros((take, systems, k), dtype=np.float64) if has_phi else None
    if take:
        _check(call(rows.ctypes.data, rec.ctypes.data, index.ctypes.data, phi.ctypes.data if has_phi else None, take,
                    ctypes.byref(n), ctypes.byref(cols)))
    out = {"step": rows["step"].copy(), "n_bodies": rows["n_bodies"].copy(), "index": index}
    for f in TRACK_FIELDS:
        out[f] = np.ascontiguousarray(rec[f])
    if has_phi:
        out["phi"] = phi
    return out


class Stepper:
    """Device-resident stepper: the loop body of src/nbody.cu:460-545 without the per-step host round trip."""

    def __init__(self, cfg=None, capacity=None, precision=F32, semantics=LITERAL, device=0, rank=0, world=1,
                 record_events=False, group=False, comm_id=None, timestep=None, growthRate=None,
                 fieldWidth=None, fieldHeight=None, event_capacity=0, kernel_variant=0, force_comm=False,
                 track_ids=False):
        d = _CtxDesc()
        if cfg is not None:
            lib.nbody_ctx_desc_from_config(ctypes.byref(d), ctypes.byref(cfg), precision)
        d.precision, d.semantics, d.device, d.rank, d.world = precision, semantics, device, rank, world
        if capacity is not None:
            d.capacity = capacity
        for name, val in (("timestep", timestep), ("growthRate", growthRate), ("fieldWidth", fieldWidth),
                          ("fieldHeight", fieldHeight)):
            if val is not None:
                setattr(d, name, val)
        d.flags = ((FLAG_RECORD_EVENTS if record_events else 0) | (FLAG_GROUP_EXCHANGE if group else 0) |
                   (FLAG_FORCE_COMM if force_comm else 0) | (FLAG_TRACK_IDS if track_ids else 0))
        d.event_capacity = event_capacity
        d.kernel_variant = kernel_variant
        self._comm_id = ctypes.create_string_buffer(comm_id, COMM_ID_BYTES) if comm_id else None
        d.comm_id = ctypes.cast(self._comm_id, ctypes.c_void_p) if self._comm_id else None
        self.precision = precision
        self.capacity = d.capacity
        self.world, self.rank = world, rank
        self._field = (d.fieldWidth, d.fieldHeight) if d.fieldWidth > 0 and d.fieldHeight > 0 else None
        self._tracks = (0, False)                               # (samples, potential) of the track log's reservation
        self._tracks_all = False                                # reserved with ids=None: tracks() trims to the uploaded count
        self._uploaded = 0
        self._ctx = ctypes.c_void_p()
        _check(lib.nbody_ctx_create(ctypes.byref(self._ctx), ctypes.byref(d)))

    def close(self):
        if getattr(self, "_ctx", None) and lib is not None:     # `lib` is gone at interpreter shutdown
            lib.nbody_ctx_destroy(self._ctx)
            self._ctx = None

    def render_image(self, width, height):
        """cudaMemset(254) + generateImage + D2H, src/nbody.cu:531-537."""
        img = np.zeros((height, width), dtype=np.uint8)
        _check(lib.nbody_render_image(self._ctx, img.ctypes.data, width, height))
        return img

    def save_state(self, path):
        _check(lib.nbody_state_save(self._ctx, os.fsencode(path)))

    def load_state(self, path):
        _check(lib.nbody_state_load(self._ctx, os.fsencode(path)))
        self._uploaded = self.body_count()                      # a load is an upload: identities restart

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def upload(self, bodies):
        """BodiesData::uploadToDevice, src/nbody.cu:88-96."""
        assert bodies.precision == self.precision
        _check(lib.nbody_upload(self._ctx, bodies.ptr, bodies.numBodies))
        self._uploaded = bodies.numBodies

    def step(self, nsteps=1, track_every=0):
        """nsteps steps, enqueue only.  track_every = k > 0: a row of the track log after every k-th step of this call
        (for i in 1..nsteps: step(1); if i % k == 0: record_tracks()), enqueue only as well."""
        if track_every < 0:
            raise ValueError("track_every %d" % track_every)
        if not track_every:
            _check(lib.nbody_step(self._ctx, nsteps))
            return
        done = 0
        while done < nsteps:
            chunk = min(track_every, nsteps - done)
            _check(lib.nbody_step(self._ctx, chunk))
            done += chunk
            if done % track_every == 0:
                _check(lib.nbody_track_record(self._ctx))

    def reserve_tracks(self, samples, ids=None, potential=False):
        """Room for `samples` rows of the track log on the device (0 frees it); empties the log.  ids: the identities to
        follow, strictly increasing (None: every identity 0 .. capacity-1); potential: keep the per-body potential too.
        Needs track_ids=True."""
        self._tracks = _reserve_tracks(lambda *a: lib.nbody_track_reserve(self._ctx, *a), samples, ids, potential)
        self._tracks_all = ids is None

    def record_tracks(self):
        """Enqueues one row of the track log: no copy, no host wait."""
        _check(lib.nbody_track_record(self._ctx))

    def tracks(self):
        """The track log, a dict of numpy arrays of shape (recorded, columns): index (current index of the identity, -1:
        absent), x, y, vx, vy, m, r (0 where absent), phi (if reserved with potential=True); step and n_bodies of shape
        (recorded,).  Reserved with ids=None, the columns are trimmed to the uploaded count.  Synchronises."""
        out = _tracks(lambda *a: lib.nbody_track_read(self._ctx, *a), self._tracks, 1, self.precision)
        out = {k: v[:, 0] for k, v in out.items()}
        if self._tracks_all:
            for k in out:
                if out[k].ndim == 2:
                    out[k] = np.ascontiguousarray(out[k][:, :self._uploaded])
        return out

    def sync(self):
        _check(lib.nbody_sync(self._ctx))

    def download(self):
        out = BodiesData(0, self.precision, self.capacity)
        n = ctypes.c_int(0)
        _check(lib.nbody_download(self._ctx, out.ptr, ctypes.byref(n)))
        out.numBodies = n.value
        return out

    def body_count(self):
        n = ctypes.c_int(0)
        _check(lib.nbody_body_count(self._ctx, ctypes.byref(n)))
        return n.value

    def own_range(self):
        lo, cnt = ctypes.c_int(0), ctypes.c_int(0)
        _check(lib.nbody_own_range(self._ctx, ctypes.byref(lo), ctypes.byref(cnt)))
        return lo.value, cnt.value

    def events(self, cap=1 << 20):
        buf = np.zeros(cap, dtype=EVENT_DTYPE)
        total = ctypes.c_int64(0)
        _check(lib.nbody_get_events(self._ctx, buf.ctypes.data, cap, ctypes.byref(total)))
        if total.value > cap:
            raise NbodyError(-7, "event log holds %d events, buffer %d" % (total.value, cap))
        return buf[:total.value]

    def clear_events(self):
        _check(lib.nbody_clear_events(self._ctx))

    def ids(self):
        """nbody_get_ids (track_ids=True): int32[n], ids()[i] = index that current body i had in the last upload."""
        return _ids(lambda buf, cap, n: lib.nbody_get_ids(self._ctx, buf, cap, n), self.capacity)

    def lineage(self, cap=1 << 20):
        """nbody_get_lineage (track_ids=True and record_events=True): a LINEAGE_DTYPE array, record k is events()[k]
        with the identities that its i and j had in that step."""
        return _lineage(lambda buf, c, total: lib.nbody_get_lineage(self._ctx, buf, c, total), cap)

    def force_kernel_name(self):
        return lib.nbody_force_kernel_name(self._ctx).decode()

    def set_kernel_timing(self, enable=True):
        _check(lib.nbody_set_kernel_timing(self._ctx, int(enable)))

    def force_only(self, reps):
        _check(lib.nbody_debug_force_only(self._ctx, reps))

    def ring_probe(self):
        out = (ctypes.c_uint64 * 8)()
        _check(lib.nbody_debug_ring_probe(self._ctx, ctypes.byref(out)))
        return list(out)

    def screen_state(self):
        """nbody_debug_screen_state: (Meta::summary, the per-tile largest |radius| the context keeps, float32)."""
        summary, n_tiles = ctypes.c_int(0), ctypes.c_int(0)
        _check(lib.nbody_debug_screen_state(self._ctx, None, None, 0, ctypes.byref(n_tiles)))
        rmax = np.zeros(n_tiles.value, dtype=np.float32)
        _check(lib.nbody_debug_screen_state(self._ctx, ctypes.byref(summary), rmax.ctypes.data, n_tiles.value, None))
        return summary.value, rmax

    def diagnostics(self, potential=False):
        """nbody_get_diagnostics: mass, momentum, center_of_mass, angular_momentum, kinetic, potential (fp64) and
        coincident_pairs of the current state; with potential=True also "phi", the per-body potential (n float64)."""
        return _diagnostics(lambda d, phi: lib.nbody_get_diagnostics(self._ctx, d, phi), self.capacity, potential)

    def field(self, points=None):
        """nbody_get_field: acceleration and potential (fp64) of the current bodies at `points` (m, 2), or with
        points=None at the bodies' own positions (self term left out): {"acc": (m, 2), "phi": (m,), "coincident": sources
        at distance 0, left out and counted}; m is the current body count for points=None, where "phi" has the bits of
        diagnostics(potential=True)["phi"].  Not collective: any rank of any world may call it on its own."""
        return _field(lambda *a: lib.nbody_get_field(self._ctx, *a), points, self.capacity)

    def tides(self, points=None, point_vel=None, jerk=False):
        """nbody_get_tides: the tidal tensor da/dx (fp64) of the current bodies at `points` (m, 2), or with points=None at
        the bodies' own positions (self term left out): {"tide": (m, 3) txx, txy, tyy, "coincident": sources at distance 0,
        left out and counted}; with jerk=True also "jerk": (m, 2), da/dt along the motion - of the bodies with their own
        velocities, of points with `point_vel` (m, 2; None: at rest).  The tensor alone is not collective: any rank of any
        world may call it on its own; jerk=True needs a single-rank context.  "tide" has the same bits either way."""
        return _tides(lambda *a: lib.nbody_get_tides(self._ctx, *a), points, point_vel, jerk, self.capacity)

    def set_tracers(self, pos, vel=None, walls=False):
        """nbody_tracers_set: m massless tracers at `pos` (m, 2) with velocities `vel` (m, 2; None: zeros), fp64 whatever
        the precision, advanced inside every later step from the field of the state the step starts from.  walls=True:
        they reflect at the field's walls by the bodies' rule.  Replaces earlier tracers and zeroes their counters."""
        rec = _tracer_records(pos, vel)
        _check(lib.nbody_tracers_set(self._ctx, rec.ctypes.data, len(rec), TRACER_WALLS if walls else 0))

    def clear_tracers(self):
        """Removes the tracers and frees their memory."""
        _check(lib.nbody_tracers_set(self._ctx, None, 0, 0))

    def tracers(self):
        """nbody_tracers_get: {"pos": (m, 2), "vel": (m, 2), "acc": (m, 2), "phi": (m,), "steps", "coincident"} - the
        tracers, the field of their most recent advance, the advances since set_tracers and the sources at distance 0 left
        out over them.  Synchronises."""
        info = np.zeros(1, dtype=TRACER_INFO_DTYPE)
        _check(lib.nbody_tracers_get(self._ctx, None, None, 0, info.ctypes.data))
        m = int(info["count"][0])
        rec, last = np.zeros(max(m, 1), dtype=TRACER_DTYPE), np.zeros(max(m, 1), dtype=FIELD_DTYPE)
        _check(lib.nbody_tracers_get(self._ctx, rec.ctypes.data, last.ctypes.data, m, info.ctypes.data))
        return _tracer_dict(rec[:m], last[:m], {k: int(info[k][0]) for k in ("steps", "coincident")})

    def neighbors(self, points=None):
        """nbody_get_neighbors: for every row - each of `points` (m, 2), or with points=None each current body (self term
        left out) - a record {"d2": squared distance to the nearest current body (fp64; +inf if there is none), "index":
        that body (-1), "overlaps": how many bodies satisfy d2 <= (r + r_j)^2 with the row (r = 0 for a point)}, as a
        NEIGHBOR_DTYPE array.  Not collective: any rank of any world may call it on its own."""
        return _neighbors(lambda *a: lib.nbody_get_neighbors(self._ctx, *a), points, self.capacity)

    def knn(self, k, points=None, grid=None, h0=None, max_radius=None, squared=False):
        """nbody_get_knn: for every row - each of `points` (m, 2), or with points=None each current body (self term left
        out by index) - the k nearest current bodies under (d2, index) ascending, 1 <= k <= KNN_MAX: {"d2": float64
        (rows, k) squared distances, "index": int32 (rows, k)}, entries past the last eligible source {+inf, -1}.  Entry 0
        has the bits of neighbors().  Not collective: any rank of any world may call it on its own.
        grid (a make_grid record, or what make_grid accepts; knn_grid() makes a matched one): nbody_get_knn_grid, the same
        entries found through the cell list in O(n), among the bodies inside the grid only; the dict gains "info": n, rows,
        inside, outside, widened, rounds and "grid".  h0: the radius of a row's first window (None: the larger cell side),
        doubled until the row has its k; max_radius: only sources within it (a length; a squared length with squared=True;
        None: no cut) - it needs a grid, the brute-force call has no cut."""
        if grid is not None:
            g = make_grid(grid)
            d2, index, info, _ = _knn_grid(lambda *a: lib.nbody_get_knn_grid(self._ctx, *a), None, self.capacity, k, points, g, h0,
                                           max_radius, squared)
            return _knn_grid_dict(d2[0], index[0], info[0], g)
        if max_radius is not None or h0 is not None:
            raise ValueError("knn(): max_radius and h0 need a grid - the brute-force call has no cut and no window")
        pts = _field_points(points)
        k = int(k)
        m = self.capacity if pts is None else len(pts)
        d2, index = _knn_buffers((max(m, 1), max(k, 1)))
        n = ctypes.c_int(0)
        _check(lib.nbody_get_knn(self._ctx, None if pts is None else pts.ctypes.data, m, k, d2.ctypes.data,
                                 index.ctypes.data, ctypes.byref(n)))
        return {"d2": d2[:n.value].copy(), "index": index[:n.value].copy()}

    def shells(self, edges, points=None, squared=False):
        """nbody_get_shells: for every row - each of `points` (m, 2), or with points=None each current body (self term left
        out by index) - the mass and the number of the current bodies in each bin of distance between the B + 1 `edges`
        (lengths; squared lengths with squared=True), 1 <= B <= SHELLS_MAX: {"mass": float64 (rows, B), summed in ascending
        index, "count": int32 (rows, B), "edges2": the squared edges that were sent}.  A source counts in bin k where
        edges2[k] <= d2 < edges2[k+1], and nowhere otherwise.  shell_profile() turns it into densities and enclosed masses.
        Not collective: any rank of any world may call it on its own."""
        e2 = pair_edges2(edges, squared)
        pts = _field_points(points)
        bins = len(e2) - 1
        m = self.capacity if pts is None else len(pts)
        mass, count = _shell_buffers((max(m, 1), bins))
        n = ctypes.c_int(0)
        _check(lib.nbody_get_shells(self._ctx, None if pts is None else pts.ctypes.data, m, e2.ctypes.data, bins,
                                    mass.ctypes.data, count.ctypes.data, ctypes.byref(n)))
        return {"mass": mass[:n.value].copy(), "count": count[:n.value].copy(), "edges2": e2}

    def shell_moments(self, edges, points=None, point_vel=None, squared=False):
        """nbody_get_shell_moments: shells() with the velocities.  For every row - each of `points` (m, 2) moving with
        `point_vel` (m, 2; None: at rest), or with points=None each current body with its own velocity (self term left out
        by index) - and each bin between the B + 1 `edges` (lengths; squared lengths with squared=True), nine fp64 sums
        over the bin's sources in ascending index and their number: {"moments": SHELL_MOMENT_DTYPE (rows, B) - mass, px, py,
        ke, mr2, rad, ang, rad2, ang2, count - "edges2": the squared edges that were sent}.  1 <= B <= 32: the library takes
        SHELL_MOMENTS_MAX bins a call, more are split into calls over adjoining edges, which gives the same bits bin for
        bin.  shell_kinematics() turns the sums into mean velocities, dispersions and rates.  Needs a single-rank context."""
        e2 = pair_edges2(edges, squared)
        pts, vel = _shell_moment_rows(points, point_vel)
        m = self.capacity if pts is None else len(pts)
        n = ctypes.c_int(0)
        mom = _shell_moments(lambda edges2, bins, out: lib.nbody_get_shell_moments(
            self._ctx, None if pts is None else pts.ctypes.data, None if vel is None else vel.ctypes.data, m, edges2, bins, out,
            ctypes.byref(n)), (max(m, 1),), e2)
        return {"moments": mom[:n.value].copy(), "edges2": e2}

    def cells(self, grid_or_nx, ny=None, bounds=None, moments=True, lists=False):
        """nbody_get_cells: for every cell of a uniform grid - make_grid(nx, ny, bounds), or a grid made by it; bounds=None:
        the field, [-fieldWidth, fieldWidth) x [-fieldHeight, fieldHeight) - the number, the mass and (moments=True) the
        momentum and twice the kinetic energy of the current bodies in it, summed in ascending index: {"cells": CELL_DTYPE
        (ny, nx) - mass, px, py, k2, count, first - "grid", "info": n, inside, outside, occupied, largest, largest_cell}; with
        lists=True also "cell_of": int32 (n,), the cell of every body (-1: outside), "start": int32 (nx*ny + 1,) and "order":
        int32 (inside,), the bodies in cell order, ascending inside a cell.  cell_maps() turns the sums into maps.
        moments=False is not collective: any rank of any world may call it; moments=True needs a single-rank context."""
        grid = _cells_grid(grid_or_nx, ny, bounds, self._field)
        cells, cell_of, start, order, info = _cells(
            lambda g, flags, c, co, st, od, inf: lib.nbody_get_cells(self._ctx, g, flags, c, co, st, od, self.capacity, inf),
            None, self.capacity, grid, moments, lists)
        return _cells_dict(cells[0], None if cell_of is None else cell_of[0], None if start is None else start[0],
                           None if order is None else order[0], info[0], grid)

    def within(self, radius, points=None, grid=None, squared=False, lists=False):
        """nbody_get_within: everything within `radius` (a length; a squared length with squared=True; inf allowed) of every
        row - each of `points` (m, 2), or with points=None each current body (its own term left out by index) - found
        through the cell list of `grid` (a make_grid record; None: within_grid(field, radius)) in O(n) where the cells are
        about `radius` wide: {"rows": a WITHIN_DTYPE array {"d2", "index": the nearest source within the radius (+inf, -1:
        none), "count": the sources within it, "overlaps": those of them with d2 <= (r + r_j)^2, "cell": the row's own cell,
        -1 outside the grid}, "info": total, n, rows, inside, outside, largest, largest_row, "grid"}; with lists=True also
        "start": int64 (rows + 1,) and "list": int32 (total,), the sources within the radius of row k in ascending index at
        list[start[k]:start[k+1]].  Only bodies inside the grid are sources; apart from "cell" the result does not depend on
        the grid otherwise.  Not collective: any rank of any world may call it on its own."""
        g = within_grid(_field_bounds(self._field)[1::2], radius, squared) if grid is None else make_grid(grid)
        return _within(lambda *a: lib.nbody_get_within(self._ctx, *a), None, self.capacity, radius, points, g, squared, lists)[0]

    def groups(self, link, radius_scale=1.0, grid=None):
        """nbody_get_groups: friends-of-friends groups of the current bodies, i and j linked where d2 <= s*s with
        s = radius_scale * (r_i + r_j) + link (fp64): {"label": int32 (n,), label[i] the lowest index of body i's group,
        "n_groups", "largest": the size of the biggest group, "sweeps": pair walks the call took}.  (0, 1) links the
        overlapping bodies of neighbors(); radius_scale=0 is friends-of-friends on the centres.  Not collective.
        grid (a make_grid record, or what make_grid accepts; groups_grid() makes a matched one): nbody_get_groups_grid, the
        same labels found through the cell list in O(n) per sweep, among the bodies inside the grid only - a body outside
        is a group of its own; the dict also has "inside", "outside" and "grid".  With outside == 0 the labels are those of
        grid=None, whatever the grid."""
        label = np.zeros(max(self.capacity, 1), dtype=np.int32)
        if grid is not None:
            g = make_grid(grid)
            info = np.zeros(1, dtype=GROUPS_GRID_INFO_DTYPE)
            _check(lib.nbody_get_groups_grid(self._ctx, g.ctypes.data, link, radius_scale, label.ctypes.data, self.capacity,
                                             info.ctypes.data))
            return _groups_grid_dict(label[:int(info["n_bodies"][0])].copy(), info[0], g)
        info = np.zeros(1, dtype=GROUPS_INFO_DTYPE)
        _check(lib.nbody_get_groups(self._ctx, link, radius_scale, label.ctypes.data, self.capacity, info.ctypes.data))
        return _groups_dict(label[:int(info["n_bodies"][0])].copy(), info[0])

    def group_potential(self, link, radius_scale=1.0):
        """nbody_get_group_potential: groups() and, for every current body, "phi": the potential (fp64) due to the other
        members of its own group only, with the bits diagnostics(potential=True) gives for a context that holds exactly the
        group's members in ascending order -> {"label", "phi", "n_groups", "largest", "sweeps", "coincident": ordered
        pairs of one group at distance 0, left out}.  Not collective."""
        label = np.zeros(max(self.capacity, 1), dtype=np.int32)
        phi = np.zeros(max(self.capacity, 1), dtype=np.float64)
        info = np.zeros(1, dtype=GROUP_ENERGY_INFO_DTYPE)
        _check(lib.nbody_get_group_potential(self._ctx, link, radius_scale, label.ctypes.data, phi.ctypes.data, self.capacity,
                                             info.ctypes.data))
        n = int(info["n_bodies"][0])
        return _group_potential_dict(label[:n].copy(), phi[:n].copy(), info[0])

    def group_energies(self, link, radius_scale=1.0):
        """group_potential(), a download and group_catalog(): one GROUP_RECORD_DTYPE record per group, sorted by label - is
        the group held together by its own gravity?  Single-rank contexts only: a rank holds only its own velocities."""
        if self.world > 1:
            raise NbodyError(-9, "group_energies: a single-rank context is needed (world %d): a rank holds only its own "
                                 "velocities, a catalogue across ranks is not built" % self.world)
        g = self.group_potential(link, radius_scale)
        return _group_energies(self.download(), g)

    def pair_counts(self, edges, points=None, squared=False, grid=None):
        """nbody_get_pair_counts: the number of pairs in each bin of separation between the B + 1 `edges` (lengths; squared
        lengths with squared=True) - the unordered pairs of current bodies, or with `points` (m, 2) every (point, body)
        pair -> {"counts": uint64 (B,), "below": pairs under the first edge, "rest": pairs at or above the last (or NaN),
        "pairs": all of them, "n_bodies", "edges2": the squared edges that were sent}.  Not collective.
        grid (a make_grid record, or what make_grid accepts): nbody_get_pair_counts_grid, the same counts found through the
        cell list in O(n), among the bodies inside the grid only; the dict also has "inside", "outside" and "grid".  With
        outside == 0 the numbers are those of grid=None, whatever the grid.  The matched grid is
        within_grid(field, top_edge): cells no smaller than the last edge."""
        if grid is not None:
            g = make_grid(grid)
            return _pair_counts(lambda *a: lib.nbody_get_pair_counts_grid(self._ctx, g.ctypes.data, *a), 1, edges, points,
                                squared, g)[0]
        return _pair_counts(lambda *a: lib.nbody_get_pair_counts(self._ctx, *a), 1, edges, points, squared)[0]

    def encounters(self, horizon=None, cap=None, grid=None):
        """nbody_get_encounters: the pairs of current bodies that touch within the next `horizon` seconds if every body keeps
        its velocity (the uniform-motion estimate: no acceleration, no walls) -> (an ENCOUNTER_DTYPE array {"t": time of
        contact, "i" < "j", "flags": ENCOUNTER_NOW | ENCOUNTER_END} sorted by (t, i, j), {"n_bodies", "pairs", "now", "end",
        "missed", "horizon"}); a pair with neither flag touches strictly inside the horizon and overlaps at neither end.
        horizon=None: the context's own time step, widened as the tracers widen it.  cap: the first guess of the room (None:
        the capacity); a longer list is fetched with a second call.  Single-rank contexts only.
        grid (a make_grid record, or what make_grid accepts): nbody_get_encounters_grid, the same list found through the
        cell list in O(n), among the bodies inside the grid only; the info dict also has "inside", "outside" and "grid".
        With outside == 0 the list and the counts are those of grid=None, whatever the grid.  The matched grid is
        encounters_grid(field, horizon, r_typical, v_typical)."""
        if horizon is None:
            d, steps = _CtxDesc(), ctypes.c_int64(0)
            _check(lib.nbody_ctx_info(self._ctx, ctypes.byref(d), ctypes.byref(steps)))
            horizon = float(np.float32(d.timestep)) if self.precision == F32 else float(d.timestep)
        cap = max(self.capacity, 64) if cap is None else cap
        if grid is not None:
            g = make_grid(grid)
            return _encounters(lambda *a: lib.nbody_get_encounters_grid(self._ctx, g.ctypes.data, *a), 1, float(horizon), cap, g)[0]
        return _encounters(lambda *a: lib.nbody_get_encounters(self._ctx, *a), 1, float(horizon), cap)[0]

    def binaries(self, max_sep, squared=False, cap=None, grid=None):
        """nbody_get_binaries: the pairs of current bodies no further apart than `max_sep` (a length; a squared length with
        squared=True; inf allowed) that are gravitationally bound as an isolated two-body system -> (a BINARY_DTYPE array
        {"a": semi-major axis, "ecc", "period", "sep": the separation now, "i" < "j", "flags": BINARY_OVERLAP |
        BINARY_APPROACHING} sorted by (i, j), {"n_bodies", "pairs", "near": all pairs within max_sep, "coincident",
        "overlapping", "approaching", "sep2"}).  cap: the first guess of the room (None: the capacity); a longer list is
        fetched with a second call.  Single-rank contexts only.
        grid (a make_grid record, or what make_grid accepts): nbody_get_binaries_grid, the same list found through the cell
        list in O(n), among the bodies inside the grid only; the info dict also has "inside", "outside" and "grid".  With
        outside == 0 the list and the counts are those of grid=None, whatever the grid.  The matched grid is
        within_grid(field, max_sep): cells no smaller than the separation."""
        cap = max(self.capacity, 64) if cap is None else cap
        if grid is not None:
            g = make_grid(grid)
            return _binaries(lambda *a: lib.nbody_get_binaries_grid(self._ctx, g.ctypes.data, *a), 1, max_sep, squared, cap, g)[0]
        return _binaries(lambda *a: lib.nbody_get_binaries(self._ctx, *a), 1, max_sep, squared, cap)[0]

    def stats(self):
        s = Stats()
        _check(lib.nbody_get_stats(self._ctx, ctypes.byref(s)))
        return s


class StepperGroup:
    """All ranks of a partition as contexts of this process (nbody_group_step): one per device, or several
    on one device.  The exchange is stream-ordered peer copies, no RCCL."""

    def __init__(self, world, devices=None, **kw):
        devices = devices or [0] * world
        self.world = world
        self.ranks = [Stepper(rank=g, world=world, device=devices[g], group=world > 1, **kw)
                      for g in range(world)]
        self._arr = (ctypes.c_void_p * world)(*[r._ctx for r in self.ranks])
        self.precision = self.ranks[0].precision
        self.capacity = self.ranks[0].capacity

    def upload(self, bodies):
        for r in self.ranks:
            r.upload(bodies)

    def step(self, nsteps=1):
        _check(lib.nbody_group_step(self._arr, self.world, nsteps))

    def download(self):
        out = BodiesData(0, self.precision, self.capacity)
        n = ctypes.c_int(0)
        _check(lib.nbody_group_download(self._arr, self.world, out.ptr, ctypes.byref(n)))
        out.numBodies = n.value
        return out

    def diagnostics(self, potential=False):
        """nbody_group_diagnostics: as Stepper.diagnostics, for the whole group."""
        return _diagnostics(lambda d, phi: lib.nbody_group_diagnostics(self._arr, self.world, d, phi), self.capacity,
                            potential)

    def field(self, points=None, rank=0):
        """Stepper.field through one rank: every rank's replica holds every position and mass, each gives the same bits."""
        return self.ranks[rank].field(points)

    def tides(self, points=None, rank=0):
        """Stepper.tides (the tensor only: a rank holds only its own velocities) through one rank: each gives the same
        bits."""
        return self.ranks[rank].tides(points)

    def neighbors(self, points=None, rank=0):
        """Stepper.neighbors through one rank: every rank's replica holds every body, each gives the same bits."""
        return self.ranks[rank].neighbors(points)

    def knn(self, k, points=None, rank=0, grid=None, h0=None, max_radius=None, squared=False):
        """Stepper.knn through one rank, with or without a grid: every rank's replica holds every body, each gives the same
        bits."""
        return self.ranks[rank].knn(k, points, grid, h0, max_radius, squared)

    def shells(self, edges, points=None, squared=False, rank=0):
        """Stepper.shells through one rank: every rank's replica holds every body, each gives the same bits."""
        return self.ranks[rank].shells(edges, points, squared)

    def cells(self, grid_or_nx, ny=None, bounds=None, moments=False, lists=False, rank=0):
        """Stepper.cells through one rank, moments=False only (a rank holds only its own velocities): every rank's replica
        holds every position and mass, each gives the same bits."""
        return self.ranks[rank].cells(grid_or_nx, ny, bounds, moments, lists)

    def within(self, radius, points=None, grid=None, squared=False, lists=False, rank=0):
        """Stepper.within through one rank: every rank's replica holds every position and radius, each gives the same bits."""
        return self.ranks[rank].within(radius, points, grid, squared, lists)

    def groups(self, link, radius_scale=1.0, rank=0, grid=None):
        """Stepper.groups through one rank, with or without a grid: every rank's replica holds every body, each gives the
        same labels."""
        return self.ranks[rank].groups(link, radius_scale, grid)

    def group_potential(self, link, radius_scale=1.0, rank=0):
        """Stepper.group_potential through one rank: every rank's replica holds every position and mass."""
        return self.ranks[rank].group_potential(link, radius_scale)

    def pair_counts(self, edges, points=None, squared=False, rank=0, grid=None):
        """Stepper.pair_counts through one rank, with or without a grid: every rank's replica holds every body, each gives
        the same numbers."""
        return self.ranks[rank].pair_counts(edges, points, squared, grid)

    def save_state(self, path):
        """nbody_group_state_save: the group's download under the header of rank 0, the file a plain Stepper writes."""
        _check(lib.nbody_group_state_save(self._arr, self.world, os.fsencode(path)))

    def load_state(self, path):
        """Every rank loads the file (a load is an upload, and a group is uploaded rank by rank)."""
        for r in self.ranks:
            r.load_state(path)

    def close(self):
        for r in self.ranks:
            r.close()


class StepperBatch:
    """S independent systems stepped together (nbody_batch_*): S copies of the loop body of src/nbody.cu:463-510 per
    launch.  System s is bit for bit what a Stepper with the same parameters gives.  fp32 only.

    params: one (timestep, growthRate, fieldWidth, fieldHeight) tuple, or an object with those attributes (a ConfigData),
    per system; or cfg=..., the same configuration for every system."""

    def __init__(self, systems, capacity, params=None, cfg=None, semantics=LITERAL, record_events=False,
                 event_capacity=0, kernel_variant=0, device=0, precision=F32, track_ids=False):
        if params is None and cfg is not None:
            params = [cfg] * max(int(systems), 0)
        arr = None
        if params is not None:
            if len(params) != systems:
                raise ValueError("%d parameter sets for %d systems" % (len(params), systems))
            arr = (_BatchParams * max(len(params), 1))()
            for s, p in enumerate(params):
                if not isinstance(p, (tuple, list)):
                    p = (p.timestep, p.growthRate, p.fieldWidth, p.fieldHeight)
                arr[s].timestep, arr[s].growthRate, arr[s].fieldWidth, arr[s].fieldHeight = p
        self._field = (arr[0].fieldWidth, arr[0].fieldHeight) if arr is not None and len(params) > 0 else None
        d = _BatchDesc()
        d.precision, d.semantics, d.systems, d.capacity, d.device = precision, semantics, systems, capacity, device
        d.flags = (FLAG_RECORD_EVENTS if record_events else 0) | (FLAG_TRACK_IDS if track_ids else 0)
        d.event_capacity = event_capacity
        d.kernel_variant = kernel_variant
        self.systems, self.capacity, self.precision = systems, capacity, precision
        self._log_cap = 0                                       # samples reserved for the recorded series
        self._tracks = (0, False)                               # (samples, potential) of the track log's reservation
        self._b = ctypes.c_void_p()
        _check(lib.nbody_batch_create(ctypes.byref(self._b), ctypes.byref(d), arr))

    def close(self):
        if getattr(self, "_b", None) and lib is not None:     # `lib` is gone at interpreter shutdown
            lib.nbody_batch_destroy(self._b)
            self._b = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def upload(self, bodies):
        """One BodiesData per system (an empty one, BodiesData(0), leaves its system empty)."""
        if len(bodies) != self.systems:
            raise ValueError("%d bodies sets for %d systems" % (len(bodies), self.systems))
        assert all(b.precision == self.precision for b in bodies)
        ptrs = (ctypes.c_void_p * self.systems)(*[b.ptr for b in bodies])
        counts = (ctypes.c_int * self.systems)(*[b.numBodies for b in bodies])
        _check(lib.nbody_batch_upload(self._b, ptrs, counts))

    def step(self, nsteps=1, record_every=0, track_every=0):
        """nsteps ensemble steps, enqueue only.  record_every = k > 0: a sample of the recorded series after every k-th
        step of this call (for i in 1..nsteps: step(1); if i % k == 0: record_diagnostics()), enqueue only as well.
        track_every = k > 0: the same for rows of the track log (record_tracks()); both may be given."""
        if record_every < 0:
            raise ValueError("record_every %d" % record_every)
        if track_every < 0:
            raise ValueError("track_every %d" % track_every)
        if not record_every and not track_every:
            _check(lib.nbody_batch_step(self._b, nsteps))
            return
        done = 0
        while done < nsteps:
            chunk = min(nsteps - done, *[k - done % k for k in (record_every, track_every) if k])
            _check(lib.nbody_batch_step(self._b, chunk))
            done += chunk
            if record_every and done % record_every == 0:
                _check(lib.nbody_batch_diag_record(self._b))
            if track_every and done % track_every == 0:
                _check(lib.nbody_batch_track_record(self._b))

    def reserve_tracks(self, samples, ids=None, potential=False):
        """As Stepper.reserve_tracks, with the one selection for every system (None: identities 0 .. capacity-1)."""
        self._tracks = _reserve_tracks(lambda *a: lib.nbody_batch_track_reserve(self._b, *a), samples, ids, potential)

    def record_tracks(self):
        """Enqueues one row of the track log for every system: no copy, no host wait."""
        _check(lib.nbody_batch_track_record(self._b))

    def tracks(self):
        """As Stepper.tracks, with the system axis after the sample axis: (recorded, systems, columns), and step and
        n_bodies of shape (recorded, systems).  Synchronises."""
        return _tracks(lambda *a: lib.nbody_batch_track_read(self._b, *a), self._tracks, self.systems, self.precision)

    def sync(self):
        _check(lib.nbody_batch_sync(self._b))

    def diagnostics(self, potential=False):
        """nbody_batch_diagnostics: one dict per system, in the form (and with the bits) of Stepper.diagnostics; with
        potential=True also "phi", the per-body potential of the system's current bodies."""
        out = (Diag * self.systems)()
        phi = np.zeros(self.systems * self.capacity, dtype=np.float64) if potential else None
        _check(lib.nbody_batch_diagnostics(self._b, out, phi.ctypes.data if potential else None))
        res = []
        for s in range(self.systems):
            d = out[s].as_dict()
            if potential:
                d["phi"] = phi[s * self.capacity:s * self.capacity + d["n_bodies"]].copy()
            res.append(d)
        return res

    def field(self, points=None):
        """nbody_batch_get_field: Stepper.field for every system in one launch, with the one set of points for all of
        them: {"acc": (S, m, 2), "phi": (S, m), "coincident": (S,) int64}, system s having the bits a Stepper holding its
        state gives.  points=None: m is `capacity`, and the entries past a system's count are zero."""
        pts = _field_points(points)
        m = self.capacity if pts is None else len(pts)
        buf = np.zeros((self.systems, max(m, 1)), dtype=FIELD_DTYPE)
        coin = np.zeros(self.systems, dtype=np.int64)
        _check(lib.nbody_batch_get_field(self._b, None if pts is None else pts.ctypes.data, m, buf.ctypes.data,
                                         coin.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return {"acc": np.ascontiguousarray(buf["acc"][:, :m]), "phi": np.ascontiguousarray(buf["phi"][:, :m]),
                "coincident": coin}

    def tides(self, points=None, point_vel=None, jerk=False):
        """nbody_batch_get_tides: Stepper.tides for every system in one launch, with the one set of points and point
        velocities for all of them: {"tide": (S, m, 3), ["jerk": (S, m, 2),] "coincident": (S,) int64}, system s having the
        bits a Stepper holding its state gives.  points=None: m is `capacity`, and the entries past a system's count are
        zero."""
        pts, vel = _tide_points(points, point_vel, jerk)
        m = self.capacity if pts is None else len(pts)
        tide = np.zeros((self.systems, max(m, 1)), dtype=TIDE_DTYPE)
        jk = np.zeros((self.systems, max(m, 1), 2), dtype=np.float64) if jerk else None
        coin = np.zeros(self.systems, dtype=np.int64)
        _check(lib.nbody_batch_get_tides(self._b, None if pts is None else pts.ctypes.data,
                                         None if vel is None else vel.ctypes.data, m, tide.ctypes.data,
                                         jk.ctypes.data if jerk else None, coin.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        out = {"tide": tide.view(np.float64).reshape(self.systems, -1, 3)[:, :m].copy(), "coincident": coin}
        if jerk:
            out["jerk"] = np.ascontiguousarray(jk[:, :m])
        return out

    def set_tracers(self, pos, vel=None, walls=False):
        """nbody_batch_tracers_set: Stepper.set_tracers for every system, the same m each: pos and vel of shape (S, m, 2);
        a (m, 2) input is given to every system."""
        rec = _tracer_records(pos, vel, self.systems)
        _check(lib.nbody_batch_tracers_set(self._b, rec.ctypes.data, rec.shape[1], TRACER_WALLS if walls else 0))

    def clear_tracers(self):
        """Removes the tracers and frees their memory."""
        _check(lib.nbody_batch_tracers_set(self._b, None, 0, 0))

    def tracers(self):
        """nbody_batch_tracers_get: Stepper.tracers with a leading system axis: "pos", "vel", "acc" (S, m, 2), "phi" (S, m),
        "steps" and "coincident" (S,) int64; system s has the bits a Stepper with its state and tracers gives."""
        info = np.zeros(max(self.systems, 1), dtype=TRACER_INFO_DTYPE)
        _check(lib.nbody_batch_tracers_get(self._b, None, None, info.ctypes.data))
        m = int(info["count"][0])
        rec = np.zeros((self.systems, max(m, 1)), dtype=TRACER_DTYPE)
        last = np.zeros((self.systems, max(m, 1)), dtype=FIELD_DTYPE)
        if m:
            _check(lib.nbody_batch_tracers_get(self._b, rec.ctypes.data, last.ctypes.data, info.ctypes.data))
        return _tracer_dict(rec[:, :m], last[:, :m], {k: info[k].copy() for k in ("steps", "coincident")})

    def neighbors(self, points=None):
        """nbody_batch_get_neighbors: Stepper.neighbors for every system in one launch, with the one set of points for all
        of them, system s having the bits a Stepper holding its state gives.  points=None: a list of S NEIGHBOR_DTYPE
        arrays, one record per current body of the system; otherwise one array of shape (S, m)."""
        pts = _field_points(points)
        m = self.capacity if pts is None else len(pts)
        buf = np.zeros((self.systems, max(m, 1)), dtype=NEIGHBOR_DTYPE)
        _check(lib.nbody_batch_get_neighbors(self._b, None if pts is None else pts.ctypes.data, m, buf.ctypes.data))
        if pts is None:
            return [buf[s, :int(k)].copy() for s, k in enumerate(self.counts())]
        return np.ascontiguousarray(buf[:, :m])

    def knn(self, k, points=None, grid=None, h0=None, max_radius=None, squared=False):
        """nbody_batch_get_knn: Stepper.knn for every system in one launch, with the one set of points and the one k for all
        of them, system s having the bits a Stepper holding its state gives.  points=None: a list of S dicts, one row per
        current body of the system; otherwise one dict of arrays of shape (S, m, k).
        grid: nbody_batch_get_knn_grid, one grid, h0 and max_radius for every system, the list stages and the walk one
        launch each: a list of S dicts in the form (and with the bits) Stepper.knn(grid=...) gives for the system's state."""
        if grid is not None:
            g = make_grid(grid)
            d2, index, info, _ = _knn_grid(lambda *a: lib.nbody_batch_get_knn_grid(self._b, *a), self.systems, self.capacity, k,
                                           points, g, h0, max_radius, squared)
            return [_knn_grid_dict(d2[s], index[s], info[s], g) for s in range(self.systems)]
        if max_radius is not None or h0 is not None:
            raise ValueError("knn(): max_radius and h0 need a grid - the brute-force call has no cut and no window")
        pts = _field_points(points)
        k = int(k)
        m = self.capacity if pts is None else len(pts)
        d2, index = _knn_buffers((self.systems, max(m, 1), max(k, 1)))
        _check(lib.nbody_batch_get_knn(self._b, None if pts is None else pts.ctypes.data, m, k, d2.ctypes.data,
                                       index.ctypes.data))
        if pts is None:
            return [{"d2": d2[s, :int(c)].copy(), "index": index[s, :int(c)].copy()} for s, c in enumerate(self.counts())]
        return {"d2": np.ascontiguousarray(d2[:, :m]), "index": np.ascontiguousarray(index[:, :m])}

    def shells(self, edges, points=None, squared=False):
        """nbody_batch_get_shells: Stepper.shells for every system in one launch, with the one set of edges and points for
        all of them, system s having the bits a Stepper holding its state gives.  points=None: a list of S dicts, one row
        per current body of the system; otherwise one dict of arrays of shape (S, m, B)."""
        e2 = pair_edges2(edges, squared)
        pts = _field_points(points)
        bins = len(e2) - 1
        m = self.capacity if pts is None else len(pts)
        mass, count = _shell_buffers((self.systems, max(m, 1), bins))
        _check(lib.nbody_batch_get_shells(self._b, None if pts is None else pts.ctypes.data, m, e2.ctypes.data, bins,
                                          mass.ctypes.data, count.ctypes.data))
        if pts is None:
            return [{"mass": mass[s, :int(c)].copy(), "count": count[s, :int(c)].copy(), "edges2": e2}
                    for s, c in enumerate(self.counts())]
        return {"mass": np.ascontiguousarray(mass[:, :m]), "count": np.ascontiguousarray(count[:, :m]), "edges2": e2}

    def shell_moments(self, edges, points=None, point_vel=None, squared=False):
        """nbody_batch_get_shell_moments: Stepper.shell_moments for every system in one launch (per 8 bins), with the one set
        of edges, points and point velocities for all of them, system s having the bits a Stepper holding its state gives.
        points=None: a list of S dicts, one row per current body of the system; otherwise one dict with "moments" of shape
        (S, m, B)."""
        e2 = pair_edges2(edges, squared)
        pts, vel = _shell_moment_rows(points, point_vel)
        m = self.capacity if pts is None else len(pts)
        mom = _shell_moments(lambda edges2, bins, out: lib.nbody_batch_get_shell_moments(
            self._b, None if pts is None else pts.ctypes.data, None if vel is None else vel.ctypes.data, m, edges2, bins, out),
            (self.systems, max(m, 1)), e2)
        if pts is None:
            return [{"moments": mom[s, :int(c)].copy(), "edges2": e2} for s, c in enumerate(self.counts())]
        return {"moments": np.ascontiguousarray(mom[:, :m]), "edges2": e2}

    def cells(self, grid_or_nx, ny=None, bounds=None, moments=True, lists=False):
        """nbody_batch_get_cells: Stepper.cells for every system, each stage one launch for the whole batch, with the one
        grid for all of them (bounds=None: the field of system 0), system s having the bits a Stepper holding its state
        gives: {"cells": CELL_DTYPE (S, ny, nx), "grid", "info": a CELLS_INFO_DTYPE array (S,)}; with lists=True also
        "cell_of": int32 (S, capacity), -1 past a system's count, "start": int32 (S, nx*ny + 1) and "order": int32 (S, capacity),
        -1 past a system's `inside`."""
        grid = _cells_grid(grid_or_nx, ny, bounds, self._field)
        cells, cell_of, start, order, info = _cells(
            lambda g, flags, c, co, st, od, inf: lib.nbody_batch_get_cells(self._b, g, flags, c, co, st, od, inf),
            self.systems, self.capacity, grid, moments, lists)
        out = {"cells": cells[:self.systems], "grid": grid[0].copy(), "info": info[:self.systems]}
        if lists:
            out.update(cell_of=cell_of[:self.systems], start=start[:self.systems], order=order[:self.systems])
        return out

    def within(self, radius, points=None, grid=None, squared=False, lists=False):
        """nbody_batch_get_within: Stepper.within for every system, each stage one launch for the whole batch, with the one
        grid (None: within_grid over the field of system 0, as many cells as a batch call may have), radius and set of
        points for all of them: a list of S dicts in the form (and with the bits) a Stepper holding the system's state
        gives."""
        if grid is None:
            most = int(np.sqrt((1 << 22) // max(self.systems, 1)))
            g = within_grid(_field_bounds(self._field)[1::2], radius, squared, min(most, 1024))
        else:
            g = make_grid(grid)
        return _within(lambda *a: lib.nbody_batch_get_within(self._b, *a), self.systems, self.capacity, radius, points, g,
                       squared, lists)

    def groups(self, link, radius_scale=1.0, grid=None):
        """nbody_batch_get_groups: Stepper.groups for every system, every pair walk one launch for the whole batch: a list
        of S dicts in the form (and with the labels) a Stepper holding the system's state gives.  grid: one grid for every
        system, nbody_batch_get_groups_grid - the list stages and every sweep one launch each."""
        label = np.zeros((self.systems, max(self.capacity, 1)), dtype=np.int32)
        if grid is not None:
            g = make_grid(grid)
            info = np.zeros(max(self.systems, 1), dtype=GROUPS_GRID_INFO_DTYPE)
            _check(lib.nbody_batch_get_groups_grid(self._b, g.ctypes.data, link, radius_scale, label.ctypes.data, info.ctypes.data))
            return [_groups_grid_dict(label[s, :int(info["n_bodies"][s])].copy(), info[s], g) for s in range(self.systems)]
        info = np.zeros(max(self.systems, 1), dtype=GROUPS_INFO_DTYPE)
        _check(lib.nbody_batch_get_groups(self._b, link, radius_scale, label.ctypes.data, info.ctypes.data))
        return [_groups_dict(label[s, :int(info["n_bodies"][s])].copy(), info[s]) for s in range(self.systems)]

    def group_potential(self, link, radius_scale=1.0):
        """nbody_batch_get_group_potential: Stepper.group_potential for every system, every pair walk and the potential one
        launch each for the whole batch: a list of S dicts in the form (and with the bits) a Stepper holding the system's
        state gives."""
        label = np.zeros((self.systems, max(self.capacity, 1)), dtype=np.int32)
        phi = np.zeros((self.systems, max(self.capacity, 1)), dtype=np.float64)
        info = np.zeros(max(self.systems, 1), dtype=GROUP_ENERGY_INFO_DTYPE)
        _check(lib.nbody_batch_get_group_potential(self._b, link, radius_scale, label.ctypes.data, phi.ctypes.data,
                                                   info.ctypes.data))
        return [_group_potential_dict(label[s, :int(info["n_bodies"][s])].copy(), phi[s, :int(info["n_bodies"][s])].copy(),
                                      info[s]) for s in range(self.systems)]

    def group_energies(self, link, radius_scale=1.0):
        """Stepper.group_energies for every system: a list of S GROUP_RECORD_DTYPE arrays."""
        return [_group_energies(self.download(s), g) for s, g in enumerate(self.group_potential(link, radius_scale))]

    def pair_counts(self, edges, points=None, squared=False, grid=None):
        """nbody_batch_get_pair_counts: Stepper.pair_counts for every system in one launch, with the one set of edges and
        points for all of them: a list of S dicts in the form (and with the numbers) a Stepper holding the system's state
        gives.  grid: one grid for every system, nbody_batch_get_pair_counts_grid - the list stages and the walk one launch
        each; the matched grid is within_grid(field, top_edge)."""
        if grid is not None:
            g = make_grid(grid)
            return _pair_counts(lambda *a: lib.nbody_batch_get_pair_counts_grid(self._b, g.ctypes.data, *a), self.systems, edges,
                                points, squared, g)
        return _pair_counts(lambda *a: lib.nbody_batch_get_pair_counts(self._b, *a), self.systems, edges, points, squared)

    def encounters(self, horizon, cap=None, grid=None):
        """nbody_batch_get_encounters: Stepper.encounters for every system in one launch: a list of S (array, info) pairs in
        the form (and with the bits) a Stepper holding the system's state gives.  The kernel takes ONE horizon for the whole
        batch, so it has to be given: a batch's systems may each have their own time step.
        grid: one grid for every system, nbody_batch_get_encounters_grid - the list stages and the walk one launch each; the
        matched grid is encounters_grid(field, horizon, r_typical, v_typical)."""
        cap = max(self.capacity, 64) if cap is None else cap
        if grid is not None:
            g = make_grid(grid)
            return _encounters(lambda *a: lib.nbody_batch_get_encounters_grid(self._b, g.ctypes.data, *a), self.systems,
                               float(horizon), cap, g)
        return _encounters(lambda *a: lib.nbody_batch_get_encounters(self._b, *a), self.systems, float(horizon), cap)

    def binaries(self, max_sep, squared=False, cap=None, grid=None):
        """nbody_batch_get_binaries: Stepper.binaries for every system in one launch, with the one separation for all of
        them: a list of S (array, info) pairs in the form (and with the bits) a Stepper holding the system's state gives.
        grid: one grid for every system, nbody_batch_get_binaries_grid - the list stages and the walk one launch each; the
        matched grid is within_grid(field, max_sep)."""
        cap = max(self.capacity, 64) if cap is None else cap
        if grid is not None:
            g = make_grid(grid)
            return _binaries(lambda *a: lib.nbody_batch_get_binaries_grid(self._b, g.ctypes.data, *a), self.systems, max_sep,
                             squared, cap, g)
        return _binaries(lambda *a: lib.nbody_batch_get_binaries(self._b, *a), self.systems, max_sep, squared, cap)

    def reserve_diagnostics(self, samples):
        """Room for `samples` recorded samples of every system on the device (0 frees it); empties the series."""
        _check(lib.nbody_batch_diag_reserve(self._b, samples))
        self._log_cap = samples

    def record_diagnostics(self):
        """Enqueues one sample of every system into the recorded series: no copy, no host wait."""
        _check(lib.nbody_batch_diag_record(self._b))

    def diagnostics_log(self):
        """The recorded series: a DIAG_DTYPE array of shape (recorded, systems).  Synchronises."""
        cap = self._log_cap
        buf = np.zeros((max(cap, 1), self.systems), dtype=DIAG_DTYPE)
        n = ctypes.c_int(0)
        _check(lib.nbody_batch_diag_read(self._b, buf.ctypes.data, cap, ctypes.byref(n)))
        return buf[:min(n.value, cap)].copy()

    def counts(self):
        out = np.zeros(self.systems, dtype=np.int32)
        _check(lib.nbody_batch_counts(self._b, out.ctypes.data_as(_ip)))
        return out

    def download(self, system):
        out = BodiesData(0, self.precision, self.capacity)
        n = ctypes.c_int(0)
        _check(lib.nbody_batch_download(self._b, system, out.ptr, ctypes.byref(n)))
        out.numBodies = n.value
        return out

    def download_all(self):
        return [self.download(s) for s in range(self.systems)]

    def events(self, system, cap=1 << 20):
        buf = np.zeros(cap, dtype=EVENT_DTYPE)
        total = ctypes.c_int64(0)
        _check(lib.nbody_batch_get_events(self._b, system, buf.ctypes.data, cap, ctypes.byref(total)))
        if total.value > cap:
            raise NbodyError(-7, "event log holds %d events, buffer %d" % (total.value, cap))
        return buf[:total.value]

    def ids(self, system):
        """nbody_batch_get_ids (track_ids=True): as Stepper.ids, for one system."""
        return _ids(lambda buf, cap, n: lib.nbody_batch_get_ids(self._b, system, buf, cap, n), self.capacity)

    def lineage(self, system, cap=1 << 20):
        """nbody_batch_get_lineage (track_ids=True and record_events=True): as Stepper.lineage, for one system."""
        return _lineage(lambda buf, c, total: lib.nbody_batch_get_lineage(self._b, system, buf, c, total), cap)

    def stats(self, system):
        s = Stats()
        _check(lib.nbody_batch_get_stats(self._b, system, ctypes.byref(s)))
        return s

    def kernel_name(self):
        return lib.nbody_batch_kernel_name(self._b).decode()
