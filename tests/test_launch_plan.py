"""What the launch plan decides, pinned: the parameters scrg_params_resolve fills in over the whole (W, O, lanes_per_pair) plane, and
the geometry scrg_query_launch reports for every setting of the plane tests.

tests/golden/launch_plan.json holds what the library answered before the kernel choice got one home (sha256 digests per W for the
plane, plain numbers for the geometry).  The choice itself is stated independently in tests/plane_inputs.py: kernel_class; here it is
only checked that settings of one class with the same geometry inputs share a geometry."""
import ctypes as C
import hashlib

import pytest

import scrooge_amd
from scrooge_amd import api
from tests import plane_inputs as pi
from tests.conftest import load_golden

LANES = (0, 1, 2, 4, 8, 16, 32, 64)
MW_TABLE = 256                      # genasm_kernels.h: SCRG_SWITCH_MW_TABLE (the test build only)


def resolve_plane(lib, switch):
    """-> ({W: sha256 of its records}, calls, accepted, {(W, O): (lanes_per_pair, lds_rows, waves_per_cu) at lanes_per_pair = 0})."""
    p, r = api.Params(), api.Params()
    lib.scrg_params_default(C.byref(p))
    p.reserved[0] = switch
    digests, calls, accepted, defaults = {}, 0, 0, {}
    for W in range(1, 258):
        h = hashlib.sha256()
        p.W = W
        for O in range(0, W + 1):
            p.O = O
            for g in LANES:
                p.lanes_per_pair = g
                st = lib.scrg_params_resolve(C.byref(p), C.byref(r))
                calls += 1
                rec = (W, O, g, switch, st)
                if st == 0:                  # (a refused call leaves the struct half filled)
                    accepted += 1
                    rec += (r.lanes_per_pair, r.lds_rows, r.waves_per_cu)
                    if g == 0:
                        defaults[(W, O)] = rec[5:]
                h.update(repr(rec).encode())
        digests[str(W)] = h.hexdigest()
    return digests, calls, accepted, defaults


def test_resolve_over_the_whole_plane():
    want = load_golden("launch_plan.json")["resolve"]
    digests, calls, accepted, defaults = resolve_plane(api.load_library(), 0)
    assert (calls, accepted) == (267280, 137116)
    # a few values in clear: the fixture is not the only statement
    assert defaults[(64, 33)] == (1, 12, 16)
    assert defaults[(64, 2)] == (1, 12, 8)
    assert defaults[(64, 0)] == (1, 12, 16)       # genasm_lane_mw_kernel at W = 64: the default is lowered for the `wide` form only
    for s in ((65, 1), (128, 65), (129, 1), (256, 129), (256, 1)):
        assert defaults[s] == (1, 12, 8), s
    assert (256, 0) not in defaults
    for W in range(1, 258):
        assert digests[str(W)] == want["shipped"][str(W)], "shipped library, W = %d" % W
    scrooge_amd.build_library(variant="select")
    sel = scrooge_amd.load_library("select")
    for switch in (0, MW_TABLE):
        digests = resolve_plane(sel, switch)[0]
        for W in range(1, 258):
            assert digests[str(W)] == want["select_%d" % switch][str(W)], "test build, reserved[0] = %d, W = %d" % (switch, W)


def query_all(aligner):
    """-> {"W_O": {"runs": [lds_bytes, pairs_per_wave, n_waves // n_cus], "distance": [...]}} for every setting."""
    out = {}
    for W, O in pi.SETTINGS:
        e = {}
        for mode, kw in (("runs", {}), ("distance", {"distance_only": True})):
            q = aligner.query_launch(W=W, O=O, **kw)
            assert q["n_waves"] % q["n_cus"] == 0
            e[mode] = [q["lds_bytes"], q["pairs_per_wave"], q["n_waves"] // q["n_cus"]]
        out["%d_%d" % (W, O)] = e
    return out


@pytest.mark.gpu
def test_query_launch_over_the_settings(aligner):
    want = load_golden("launch_plan.json")["query_launch"]
    got = query_all(aligner)
    assert sorted(got) == sorted(want) and len(got) == len(pi.SETTINGS)
    for key in got:
        assert got[key] == want[key], key
    # kernel_class and the fixture agree: within a class, the geometry is a function of what that kernel's LDS depends on
    # (default: nothing; halves: W <= 64 or not; parts: the words of a vector; hbm: W - O rounded up to 4 bytes, and W <= 64 — 64/0 — for the wavefronts per CU)
    depends_on = {"default": lambda W, O: (), "halves": lambda W, O: (W <= 64,), "parts": lambda W, O: ((W + 63) // 64,),
                  "hbm": lambda W, O: ((W - O + 3) // 4, W <= 64)}
    seen = {}
    for W, O in pi.SETTINGS:
        cls = pi.kernel_class(W, O)
        k = (cls,) + depends_on[cls](W, O)
        e = want["%d_%d" % (W, O)]
        assert seen.setdefault(k, e) == e, (W, O, k)
