"""The ctypes binding against include/vmm_ba.h, whole: every struct's layout as a C compiler sees the header, every
function's place and argument count in _lib.SIGNATURES, and the one place where keyword options become struct fields
(engine._set_fields).  No GPU: the header is plain C, and the default-option calls make no device call.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def _header():
    with open(os.path.join(INCLUDE, "vmm_ba.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def _header_structs():
    """{struct name: [field names in order]} for every `typedef struct vmm_ba_x { ... } vmm_ba_x;` of the header (the
    opaque handle has no body and does not match)."""
    out = {}
    for name, body in re.findall(r"typedef struct (vmm_ba_\w+) \{(.*?)\} \1;", _header(), re.S):
        out[name] = [re.search(r"(\w+)\s*(?:\[\d+\])?$", part.strip()).group(1)
                     for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    return out


def _classes():
    """{vmm_ba_snake_name: ctypes class} for every Structure of _lib: KernelTimes <-> vmm_ba_kernel_times."""
    from visual_marker_mapping_amd import _lib
    return {"vmm_ba_" + re.sub(r"(?<!^)(?=[A-Z])", "_", k).lower(): v for k, v in vars(_lib).items()
            if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure}


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    """What the host C compiler makes of the header: {"vmm_ba_x": sizeof, "vmm_ba_x.field": offsetof}.  One compile."""
    structs = _header_structs()
    lines = ['#include <stdio.h>', '#include "vmm_ba.h"', "int main(void) {"]
    for s, fields in structs.items():
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        lines += ['    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f) for f in fields]
    lines += ["    return 0;", "}", ""]
    d = tmp_path_factory.mktemp("abi_probe")
    for cc, flags in (("cc", ["-std=c99", "-x", "c"]), ("gcc", ["-std=c99", "-x", "c"]), ("g++", ["-x", "c++"])):
        if shutil.which(cc):
            break
    else:
        pytest.fail("no host C compiler (cc, gcc or g++, which tests/cpp/Makefile needs as well): the layout is unchecked")
    src, exe = str(d / "probe.c"), str(d / "probe")
    with open(src, "w") as f:
        f.write("\n".join(lines))
    subprocess.run([cc, "-Wall", "-Werror", "-I", INCLUDE] + flags + [src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_every_struct_is_laid_out_as_the_header_says(c_layout):
    structs, classes = _header_structs(), _classes()
    assert len(structs) >= 18
    assert sorted(structs) == sorted(classes)   # no struct without a class, no class without a struct
    for name, fields in structs.items():
        cls = classes[name]
        assert [f for f, _ in cls._fields_] == fields, name
        assert C.sizeof(cls) == c_layout[name], name
        for f in fields:
            assert getattr(cls, f).offset == c_layout["%s.%s" % (name, f)], (name, f)


def _header_functions():
    """{function: (return type text, number of parameters)} for every declaration of the header."""
    out = {}
    for ret, name, params in re.findall(r"^((?:const\s+)?\w+\s*\*?)\s*(vmm_ba_\w+)\s*\(([^()]*)\)\s*;", _header(), re.M):
        params = params.strip()
        out[name] = (" ".join(ret.split()), 0 if params in ("", "void") else len(params.split(",")))
    return out


def test_every_function_is_in_the_signature_table_with_its_argument_count():
    from visual_marker_mapping_amd import _lib
    declared = _header_functions()
    assert len(declared) >= 46 and declared["vmm_ba_rig_calibrate"] == ("int", 20) and declared["vmm_ba_last_error"][1] == 0
    assert sorted(declared) == sorted(_lib.SIGNATURES) == sorted(_lib.EXPORTS)
    assert _lib.OPTIONAL <= set(_lib.SIGNATURES)
    L = _lib.lib()
    for name, (ret, n_params) in declared.items():
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == n_params, name
        assert (restype is None) == (ret == "void"), name
        # and lib() has put the table on the loaded library
        assert getattr(L, name).restype is restype and list(getattr(L, name).argtypes) == argtypes, name
    assert _lib.SIGNATURES["vmm_ba_last_error"][0] is C.c_char_p


def test_set_fields_sets_known_fields_and_refuses_the_rest():
    from visual_marker_mapping_amd import _lib, engine
    o = engine._set_fields(_lib.CalibrateOptions(), dict(max_trials=7, inlier_px=2.5, loc_inlier_px=50.0, loc_robustify=0),
                           "calibration", nested=("loc_", "loc"))
    assert (o.max_trials, o.inlier_px, o.loc.inlier_px, o.loc.robustify) == (7, 2.5, 50.0, 0)
    for kw in ("no_such", "reserved", "loc_no_such", "loc"):
        for what, default in (("calibration", engine.default_calibrate_options),
                              ("rig calibration", engine.default_rig_calibrate_options)):
            with pytest.raises(AttributeError) as ei:
                default(**{kw: 1})
            assert str(ei.value) == "unknown %s option %r" % (what, kw)
    # without `nested` a prefixed name is an unknown name like any other
    for what, default, kw in (("solver", engine.default_options, "no_such"), ("solver", engine.default_options, "reserved"),
                              ("localisation", engine.default_localize_options, "loc_inlier_px"),
                              ("localisation", engine.default_localize_options, "reserved"),
                              ("triangulation", engine.default_triangulate_options, "reserved"),
                              ("triangulation", engine.default_triangulate_options, "min_inlier_tags")):
        with pytest.raises(AttributeError) as ei:
            default(**{kw: 1})
        assert str(ei.value) == "unknown %s option %r" % (what, kw)
    with pytest.raises(AttributeError) as ei:
        engine._set_fields(_lib.InitOptions(), dict(sweeps=2, reserved=1), "initialisation")
    assert str(ei.value) == "unknown initialisation option 'reserved'"
    # the defaults come from the library, the keywords on top
    assert engine.default_options(max_num_iterations=3).max_num_iterations == 3
    assert engine.default_options().huber_a == 1.0 and engine.default_triangulate_options(max_pair_views=4).max_pair_views == 4


def test_one_result_layout_serves_images_frames_and_points():
    import numpy as np
    from visual_marker_mapping_amd import _lib, engine
    arr = engine._results(3)
    assert arr.dtype.itemsize == C.sizeof(_lib.LocalizeResult) == C.sizeof(_lib.TriangulateResult) == 32
    assert arr.dtype.names == tuple(f for f, _ in _lib.TriangulateResult._fields_)
    arr["status"], arr["rms_px"] = [0, 3, 1], [0.5, 0.0, 2.0]
    dicts = engine._result_dicts(arr)
    assert [d["status"] for d in dicts] == [0, 3, 1] and dicts[2]["rms_px"] == 2.0
    assert list(dicts[0]) == ["status", "n_obs", "n_inlier_obs", "trials", "rms_px", "cost"]
    assert all(type(d["status"]) is int and type(d["cost"]) is float for d in dicts)
    assert engine._result_dicts(engine._results(0)) == [] and isinstance(arr, np.ndarray)
