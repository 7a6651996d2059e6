"""Which compiled body runs each pass of a plan (ronkathon_amd/csrc/tile_select.h, the one selection rule of the library's
launch_tile and of the fiber emulator): `emu_tile select <plan args>` builds the plan and prints its pass lines without
executing anything, so every branch of the rule is checked cheaply, for both fields, at sizes up to 2^30."""
import os
import subprocess

import pytest

from test_emu_kernel import emu, run  # noqa: F401  (the emulator fixture: builds build/emu_tile)

MONT = {"RONK_EMU_P": "0xFFFFFFFC00000001", "RONK_EMU_G": "10"}   # a Montgomery prime (> 2^63)
CFG2, CFGM, ROW = "cfg:column/two-level", "cfg:column/matrix", "cfg:row"
HALF2, HALFR = "half:column/two-level", "half:row"
WL2, WLM, WLR = "wl:column/two-level", "wl:column/matrix", "wl:row"
FEAT2, FEATR = "feat:column/two-level", "feat:row"
MUL_FWD = (20, 2, 0, 2, 18, 25, 300000, 0, 0, 700001)   # a multiply's operand pair: zero-padded input (FEAT 1)
MUL_INV = (20, 1, 1, 4, 18, 25, 0, 1000001, 1, 0, 1)     # its inverse: second operand in (FEAT 2), truncated out (FEAT 4)

# (env, plan arguments, Goldilocks labels, Montgomery labels)
CASES = [
    # the specialised shapes: column pass with two-level twiddles / the full matrix, row pass, whole polynomials
    ({}, (22, 1, 0, 4), (CFG2, ROW), (CFG2, ROW)),
    ({}, (16, 3, 0, 4, 18), (CFGM, ROW), (CFGM, ROW)),
    ({}, (12, 3, 0, 0), ("cfg:whole",), ("generic",)),
    # kind after kind: a (7, 5) column pass has no KIND 1 shape and runs the KIND 4 (DIST) one; Montgomery has no DIST shapes
    ({}, (14, 1, 0, 5), ("cfg:general", "generic"), ("generic", "generic")),
    # HALF under the grid-size rule (>= 2 * 256 * 1024 work-items; row passes only up to 2^9 rows or 2^11 x 8): Goldilocks only
    ({}, (21, 3, 0, 4), (CFG2, ROW), (CFG2, ROW)),
    ({}, (21, 4, 0, 4), (HALF2, ROW), (CFG2, ROW)),
    ({}, (22, 2, 0, 4), (HALF2, HALFR), (CFG2, ROW)),
    ({}, (22, 4, 0, 4), (HALF2, HALFR), (CFG2, ROW)),
    ({}, (19, 32, 0, 4), (HALF2, HALFR), (CFG2, ROW)),
    ({}, (20, 16, 0, 4), (HALF2, ROW), (CFG2, ROW)),
    ({"RONK_HALF_LDS": "0"}, (22, 4, 0, 4), (CFG2, ROW), (CFG2, ROW)),
    ({"RONK_HALF_LDS": "1"}, (22, 1, 0, 4), (HALF2, HALFR), (CFG2, ROW)),
    ({"RONK_HALF_LDS": "2"}, (22, 1, 0, 4), (CFG2, HALFR), (CFG2, ROW)),
    ({"RONK_HALF_LDS": "1"}, (22, 1, 1, 2), (WL2, WLR), (WL2, WLR)),
    # FEAT: Goldilocks in both directions; Montgomery only in the direction the feature occurs in, else the generic kernel
    ({}, MUL_FWD, (FEAT2, WLR), (FEAT2, WLR)),
    ({}, MUL_INV, (FEAT2, FEATR), (FEAT2, FEATR)),
    ({}, MUL_FWD[:2] + (1,) + MUL_FWD[3:], (FEAT2, WLR), ("generic", WLR)),
    ({}, (20, 1, 0, 4, 18, 25, 0, 1000001, 1), (WL2, FEATR), (WL2, "generic")),
    ({}, (16, 16, 0, 4, 18, 25, 32768, 0, 1), ("feat:column/matrix", ROW), ("feat:column/matrix", ROW)),
    # WL: 2^10 / 2^11 / 2^12-row x 4-column passes, RONK_WL, RONK_WL_ROWS, RONK_WL_HALF (Montgomery: the full image)
    ({}, (20, 1, 0, 2), (WL2, WLR), (WL2, WLR)),
    ({}, (22, 1, 1, 2), (WL2, WLR), (WL2, WLR)),
    ({}, (24, 1, 0, 2), (WL2, WLR), (WL2, WLR)),
    ({}, (21, 1, 1, 4, 21, 25, 0, 0, 1), (WLM, ROW), (WLM, ROW)),
    ({"RONK_WL": "0"}, (22, 1, 1, 2), (CFG2, ROW), (CFG2, ROW)),
    ({"RONK_WL": "2"}, (22, 1, 1, 2), (WL2, ROW), (WL2, ROW)),
    ({"RONK_WL": "3"}, (22, 1, 1, 2), (CFG2, WLR), (CFG2, WLR)),
    ({"RONK_WL_ROWS": "1"}, (22, 1, 1, 2), (CFG2, ROW), (CFG2, ROW)),
    ({"RONK_WL_ROWS": "2"}, (22, 1, 1, 2), (WL2, WLR), (WL2, WLR)),
    ({"RONK_WL_ROWS": "6"}, (20, 1, 0, 2), (CFG2, ROW), (CFG2, ROW)),
    ({"RONK_WL_ROWS": "3"}, (24, 1, 0, 2), (CFG2, ROW), ("generic", "generic")),
    ({"RONK_WL_HALF": "1"}, (22, 1, 1, 2), (WL2, WLR), (WL2, WLR)),
    ({"RONK_WL_HALF": "1"}, (22, 1, 0, 2, 22), (WLM, WLR), (WLM, WLR)),
    # the full twiddle matrix transposed (RONK_TWF_T, made only for the WL column body): WL for both fields
    ({"RONK_TWF_T": "1"}, (22, 1, 0, 2, 22), (WLM, WLR), (WLM, WLR)),
    # R4 (opt-in, Goldilocks): wins over WL at 2^10 rows, not at 2^11
    ({"RONK_R4MID": "1"}, (20, 1, 0, 2), ("r4:column/two-level", "r4:row"), (WL2, WLR)),
    ({"RONK_R4MID": "1"}, (22, 1, 1, 2), (WL2, WLR), (WL2, WLR)),
    ({"RONK_R4MID": "1"}, (18, 1, 0, 4, 18), ("r4:column/matrix", ROW), (CFGM, ROW)),
    ({"RONK_NO_CFG_KERNELS": "1"}, (22, 1, 0, 4), ("generic", "generic"), ("generic", "generic")),
    ({"RONK_NO_CFG_KERNELS": "1"}, (22, 1, 1, 2), ("generic", "generic"), ("generic", "generic")),
    # three-pass plans: the last pass has flat rows, which ntt_tile_wl.h's row body cannot read (it ran there and was wrong)
    ({}, (30, 1, 0, 2), ("generic", WL2, "generic"), ("generic", WL2, "generic")),
    ({"RONK_SPLIT3": "5,5"}, (20, 1, 0, 2, 0, 20), ("generic", "generic", ROW), ("generic", "generic", ROW)),
    ({"RONK_SPLIT3": "4,4"}, (20, 1, 0, 4, 0, 20), ("generic", "generic", ROW), ("generic", "generic", "generic")),
    ({}, (23, 1, 0, 4, 18, 23), (HALF2, "half:column/matrix", HALFR), (CFG2, CFGM, ROW)),
]


def select(emu, args, env):
    out = subprocess.run([emu, "select"] + [str(a) for a in args], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, **env))
    assert out.returncode == 0, out.stdout[-400:] + out.stderr[-400:]
    return tuple(l.split("kernel=")[1] for l in out.stdout.splitlines() if l.startswith("pass"))


@pytest.mark.parametrize("env,args,gl,mont", CASES)
def test_selection_rule(emu, env, args, gl, mont):  # noqa: F811
    assert select(emu, args, env) == gl
    assert select(emu, args, dict(env, **MONT)) == mont


@pytest.mark.parametrize("env,args", [({"RONK_SPLIT3": "5,5"}, (20, 1, 0, 2, 0, 20)), ({"RONK_SPLIT3": "4,4"}, (20, 1, 0, 4, 0, 20)),
                                      (dict(MONT, RONK_SPLIT3="5,5"), (20, 1, 1, 2, 0, 20))])
def test_three_pass_flat_rows_against_the_oracle(emu, env, args):  # noqa: F811
    """the last pass of these plans has 2^10 / 2^12 flat rows x 4 columns: it used to run the WL row body, which steps by
    (16 * RL) >> 31 = 0 blocks there, and gave wrong output"""
    out = run(emu, *args, env=env)
    assert "kernel=wl:row" not in out
