"""The diagnostic library's A/B knobs by name: ``enum gsvc_knob`` of
include/gsvc_amd_diag.h (the registry, with what each knob does), mirrored for
tests and tools -- ``lib.gsvc_debug_set(Knob.FWD_MODE, 2)``.  tests/test_capi.py
holds the two together.  ``RETIRED`` numbers belonged to finished A/Bs and are
never reused: gsvc_debug_set returns -1 for them.
"""
from enum import IntEnum


class Knob(IntEnum):
    FWD_MODE = 0
    SPARSE_MAX = 3
    STAMP = 5
    TILE_WG256 = 8
    TILE_ABLATE = 13
    TILE_NO_GROUPS = 14
    GROUP_MIN = 15
    NO_SIGMA_CUT = 19
    RECORD_SLABS = 24
    BATCH_ID_SLABS = 25
    KEEP_ORDER = 27
    ALPHA_BWD_ABLATE = 30
    SPARSE_ABLATE = 36
    GENERIC_RENDER = 38
    RENDER_STAMPS = 39


# A retired knob's name still resolves to its number (a plain attribute, not a
# member: ``for k in Knob`` is the live list), so a stale caller that names it
# stops where every retired number does -- gsvc_debug_set's -1 -- and not on
# an AttributeError while its module is imported.
Knob.SPLAT_ONE_LANE = 34

RETIRED = (1, 2, 4, 6, 7, 9, 10, 11, 12, 16, 17, 18, 20, 21, 22, 23, 26, 28, 29, 31, 32, 33, 34, 35, 37)
