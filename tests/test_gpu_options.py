"""bspgemm_set_option / bspgemm_get_option, option by option: the default, the accepted boundary values read back, the values
just outside refused with BSPGEMM_ERR_INVALID, the stored value unchanged and the refusal text in bspgemm_last_error; an
unknown option and a NULL context.  One context, no product.  The option numbers come from the header's enum; the refusal
texts are the library's, written out here so that a change of wording is a decision."""
import os
import re

import pytest

import bspgemm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = 1
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
LANES = (0, 4, 16, 64)


def _header_options():
    text = open(os.path.join(ROOT, "include", "bspgemm.h")).read()
    body = re.search(r"typedef enum bspgemm_option \{([^}]*)\}\s*bspgemm_option;", text).group(1)
    return {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"BSPGEMM_OPT_([A-Z0-9_]+)\s*=\s*(\d+)", body)}


def _shared_slots_max():
    text = open(os.path.join(ROOT, "binary-spgemm_amd", "csrc", "kernels.hpp")).read()
    return int(re.search(r"constexpr int kSharedSlotsMax = (\d+);", text).group(1))


OPT = _header_options()
# name: (default, accepted boundary values, refused values next to them, refusal text)
RANGES = {
    "class_streams": (2, (1, 3), (0, 4), "class streams: 1..3"),
    "blocked_extents": (-1, (-1, 0, 1), (-2, 2), "blocked extents: -1, 0 or 1"),
    "small_path": (-1, (-1, 0, 1), (-2, 2), "small path: -1, 0 or 1"),
    "padded_rows": (0, (-1, 0, 1), (-2, 2), "padded rows: -1, 0 or 1"),
    "dot_light": (32, (0, INT_MAX), (-1, INT_MIN), "dot light: 0 or a row length"),
    "bfs_alpha": (15, (1, INT_MAX), (0, -1, INT_MIN), "bfs alpha: 1 or more"),
    "bfs_beta": (18, (1, INT_MAX), (0, -1, INT_MIN), "bfs beta: 1 or more"),
    "lp_min_class": (0, (0, 3), (-1, 4), "lp min class: 0..3"),
    "pr_min_class": (0, (0, 3), (-1, 4), "pr min class: 0..3"),
    "bfs_push_lanes": (0, LANES, (), "bfs push lanes: 0, 4, 16 or 64"),
    "bc_lanes": (0, LANES, (), "bc lanes: 0, 4, 16 or 64"),
    "extract_lanes": (0, LANES, (), "extract lanes: 0, 4, 16 or 64"),
    "match_lanes": (0, LANES, (), "match lanes: 0, 4, 16 or 64"),
}
LANES_OPTIONS = ("bfs_push_lanes", "bc_lanes", "extract_lanes", "match_lanes")
DEFAULTS = dict({k: v[0] for k, v in RANGES.items()}, check=0, shared_slots=-1)
# what bspgemm_create reads for these fields: the defaults are those of a process that sets none of them
ENVIRONMENT = ("BSPGEMM_CLASS_STREAMS", "BSPGEMM_CHECK", "BSPGEMM_RW_BLK", "BSPGEMM_SMALL", "BSPGEMM_PAD_ROWS",
               "BSPGEMM_SHARED_SLOTS")


def test_every_option_default_bounds_and_refusals(monkeypatch):
    assert OPT == bspgemm.OPTIONS and sorted(OPT.values()) == list(range(1, 16))
    assert sorted(DEFAULTS) == sorted(OPT)
    for name in ENVIRONMENT:
        monkeypatch.delenv(name, raising=False)
    L = bspgemm.lib()
    ctx = bspgemm.Context(0)
    h = ctx._h

    def get(name):
        return L.bspgemm_get_option(h, OPT[name])

    def accepted(name, value, stored=None):
        assert L.bspgemm_set_option(h, OPT[name], value) == 0, (name, value, L.bspgemm_last_error())
        assert get(name) == (value if stored is None else stored), (name, value)

    def refused(name, value, text):
        before = get(name)
        assert L.bspgemm_set_option(h, OPT[name], value) == ERR_INVALID, (name, value)
        assert text in L.bspgemm_last_error().decode(), (name, value, L.bspgemm_last_error())
        assert get(name) == before, (name, value)

    try:
        for name, want in DEFAULTS.items():
            assert get(name) == want, name
        for name, (_default, good, bad, text) in RANGES.items():
            for v in good:
                accepted(name, v)
                for b in bad:
                    refused(name, b, text)
        for name in LANES_OPTIONS:
            for v in range(-1, 66):
                if v in LANES:
                    accepted(name, v)
                else:
                    refused(name, v, RANGES[name][3])
            for v in (INT_MIN, INT_MAX):
                refused(name, v, RANGES[name][3])
        for v, stored in ((1, 1), (0, 0), (2, 1), (-1, 1), (INT_MAX, 1), (INT_MIN, 1), (0, 0)):
            accepted("check", v, stored)
        clamp = _shared_slots_max()
        for v, stored in ((-1, -1), (0, 0), (1, 1), (clamp, clamp), (clamp + 1, clamp), (INT_MAX, clamp)):
            accepted("shared_slots", v, stored)
            for b in (-2, INT_MIN):
                refused("shared_slots", b, "shared slots: -1, 0 or a count")
        # an option the enum does not name: refused, and nothing to read
        for unknown in (0, 16):
            assert L.bspgemm_set_option(h, unknown, 1) == ERR_INVALID
            assert "unknown option" in L.bspgemm_last_error().decode()
            assert L.bspgemm_get_option(h, unknown) == INT_MIN
        # a NULL context is refused before the option is looked at
        for opt in (OPT["class_streams"], 0, 16):
            assert L.bspgemm_set_option(None, opt, 1) == ERR_INVALID
            assert "set_option: ctx is NULL" in L.bspgemm_last_error().decode()
            assert L.bspgemm_get_option(None, opt) == INT_MIN
    finally:
        for name, want in DEFAULTS.items():
            L.bspgemm_set_option(h, OPT[name], want)
        restored = {name: get(name) for name in DEFAULTS}
        ctx.close()
    assert restored == DEFAULTS
