"""The return code of every refused backward call, entry point by entry point (CPU only).

tests/golden/backward_return_codes.json holds rows (entry point, one named perturbation of an otherwise valid fake-pointer call,
return code), recorded from the library as it stood before the eight backward entry points and gsr_backward_camera were put
behind one checked request (`python tests/test_backward_abi_matrix.py --record`, on a machine without a GPU).  The test replays
every row and asks for the same code.  Every row is a REFUSED call: a perturbation that the library accepts (an optional pointer
left out, say) would carry fake pointers into a launch, so the recorder drops it and the test refuses a table that holds one.
There is no all-valid row.  One fault at a time: precedence between two faults is not pinned here."""
import ctypes as C
import json
import os
import sys

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from abi_helpers import A, fake_call_setup, libpath  # noqa: F401  (libpath: the build-if-missing fixture)
from conftest import ROOT, sub

TABLE = os.path.join(ROOT, "tests", "golden", "backward_return_codes.json")
STRUCTS = ("scene", "cam", "geom", "binning", "img", "pg", "grads")
# the arguments of each entry point, in order, by their names in the state below
ENTRIES = {
    "gsr_backward": ("scene", "cam", "geom", "binning", "img", "dpix", "grads", "ws", "ws_bytes", "stream"),
    "gsr_backward_blend": ("scene", "cam", "geom", "binning", "img", "dpix", "payload", "ws", "ws_bytes", "stream"),
    "gsr_backward_geom": ("scene", "cam", "geom", "grads", "ws", "ws_bytes", "stream"),
    "gsr_backward_aux": ("scene", "cam", "geom", "binning", "img", "pg", "grads", "inv", "ws", "ws_bytes", "stream"),
    "gsr_backward_blend_aux": ("scene", "cam", "geom", "binning", "img", "pg", "payload", "ws", "ws_bytes", "stream"),
    "gsr_backward_geom_aux": ("scene", "cam", "geom", "grads", "inv", "ws", "ws_bytes", "stream"),
    "gsr_backward_flags": ("scene", "cam", "geom", "binning", "img", "pg", "grads", "inv", "ws", "ws_bytes", "flags", "stream"),
    "gsr_backward_blend_flags": ("scene", "cam", "geom", "binning", "img", "pg", "payload", "ws", "ws_bytes", "flags", "stream"),
    "gsr_backward_camera": ("scene", "cam", "geom", "dcam", "ws", "ws_bytes", "scratch", "scratch_bytes", "stream"),
}
POINTER_ARGS = ("dpix", "payload", "inv", "ws", "dcam", "scratch")


def _valid_state():
    """Every pointer present and aligned (optional ones too), sizes exact: each entry point would accept it."""
    _lib, L, _, N, W, H, scene, cam = fake_call_setup()
    st = {"scene": scene, "cam": cam, "geom": _lib.GsrGeom(*[A] * 11), "binning": _lib.GsrBinning(100, A, A, A, A, A, 0),
          "img": _lib.GsrImage(A, A, A, A), "pg": _lib.GsrPixelGrads(A, A, A), "grads": _lib.GsrGrads(*[A] * 9),
          "ws_bytes": int(L.gsr_backward_workspace_bytes(N, 100, W, H)), "scratch_bytes": int(L.gsr_backward_camera_scratch_bytes(N)),
          "flags": 0, "stream": None}
    st.update({k: A for k in POINTER_ARGS})
    return _lib, L, st


def _pointer_members(struct):
    return [name for name, ctype in struct._fields_ if ctype is C.c_void_p]


def perturbations(args):
    """name -> list of (path, value) edits, for an entry point that takes `args`.  `+4` keeps a pointer non-NULL and misaligns it."""
    _, _, st = _valid_state()
    out = {}
    for s in STRUCTS:
        if s not in args:
            continue
        out[f"{s}=NULL"] = [(s, None)]
        for m in _pointer_members(st[s]):
            out[f"{s}.{m}=NULL"] = [(f"{s}.{m}", None)]
            out[f"{s}.{m}+4"] = [(f"{s}.{m}", A + 4)]
    for p in POINTER_ARGS:
        if p in args:
            out[f"{p}=NULL"] = [(p, None)]
            out[f"{p}+4"] = [(p, A + 4)]
    out["scene.N=-1"] = [("scene.N", -1)]
    out["scene.sh_degree=4"] = [("scene.sh_degree", 4)]
    out["cam.W=0"] = [("cam.W", 0)]
    out["ws_bytes-1"] = [("ws_bytes", st["ws_bytes"] - 1)]
    if "scratch_bytes" in args:
        out["scratch_bytes-1"] = [("scratch_bytes", st["scratch_bytes"] - 1)]
    if "binning" in args:
        out["binning.D=-1"] = [("binning.D", -1)]
        out["binning.D=2^30+1"] = [("binning.D", (1 << 30) + 1)]
        out["geom: neither records nor xy"] = [("geom.blend_records", None), ("geom.xy", None)]
    if "flags" in args:
        out["flags=2"] = [("flags", 2)]
        out["flags=0x80000001"] = [("flags", 0x80000001)]
    if "pg" in args:
        out["pg: all three NULL"] = [("pg.dL_dpixels", None), ("pg.dL_dinv_depth", None), ("pg.dL_dalpha", None)]
        out["pg.dL_dinv_depth without records or depths"] = [("geom.blend_records", None), ("geom.depths", None)]
    if "grads" in args:
        out["grads: neither dL_dshs nor dL_drgb"] = [("grads.dL_dshs", None), ("grads.dL_drgb", None)]
    return out


def call(entry, edits):
    _lib, L, st = _valid_state()
    for path, value in edits:
        head, _, member = path.partition(".")
        if member:
            setattr(st[head], member, value)
        else:
            st[head] = value
    argv = [(C.byref(st[a]) if st[a] is not None else None) if a in STRUCTS else st[a] for a in ENTRIES[entry]]
    return _lib, int(getattr(L, entry)(*argv))


def record():
    """Rows of the refused calls of the library now built.  Accepted calls end in GSR_E_HIP only where there is no GPU, so this
    refuses to run where there is one."""
    assert not os.path.exists("/dev/kfd"), "record the table on a machine without a GPU: accepted calls carry fake pointers"
    rows = []
    for entry, args in ENTRIES.items():
        for name, edits in perturbations(args).items():
            _lib, rc = call(entry, edits)
            if rc not in (_lib.GSR_OK, _lib.GSR_E_HIP):
                rows.append([entry, name, rc])
    with open(TABLE, "w") as f:
        f.write('{"rows": [\n' + ",\n".join(json.dumps(r) for r in rows) + "\n]}\n")
    return rows


def test_refused_backward_calls_return_the_recorded_codes(libpath):
    rows, _lib = json.load(open(TABLE))["rows"], sub("_lib")
    assert {r[0] for r in rows} == set(ENTRIES) and len(rows) >= 400
    seen, wrong = set(), []
    for entry, name, want in rows:
        assert (entry, name) not in seen
        seen.add((entry, name))
        assert want not in (_lib.GSR_OK, _lib.GSR_E_HIP), (entry, name)       # a refused call, by the table itself ...
        _, got = call(entry, perturbations(ENTRIES[entry])[name])
        assert got not in (_lib.GSR_OK, _lib.GSR_E_HIP), (entry, name, got)   # ... and by this build, before anything else is tried
        if got != want:
            wrong.append((entry, name, want, got))
    assert not wrong, wrong


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_backward_abi_matrix.py --record"
    print(len(record()), "rows ->", TABLE)
