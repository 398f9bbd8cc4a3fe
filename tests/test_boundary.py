"""CPU tests of the drop-in boundary: the C-ABI library loads, exports every
symbol the headers declare, and its host-side logic behaves without a GPU
(argument validation, Ceres-style problem building, loud failure instead of
a CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from ar_slam_amd import build, lm
    build.build()
    return lm


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(arslam_\w+)\s*\(", src)))


HEADERS = ["arslam_lm.h", "arslam_lm_debug.h", "arslam_localize.h", "arslam_slam.h"]
# the ctypes mirror of every struct the headers define
MIRRORS = {"arslam_lm_options": "Options", "arslam_lm_iteration": "Iteration", "arslam_lm_summary": "Summary",
           "arslam_soa_problem": "SoaProblem", "arslam_lm_cov_info": "CovInfo", "arslam_lm_cov_pair": "CovPair",
           "arslam_lm_evaluate_options": "EvaluateOptions", "arslam_tile_plan_facts": "TilePlanFacts",
           "arslam_lm_step_info": "StepInfo", "arslam_plan_info": "PlanInfo", "arslam_order_step": "OrderStep",
           "arslam_split_info": "SplitInfo", "arslam_localize_batch": "LocalizeBatchC",
           "arslam_localize_result": "LocalizeResult", "arslam_transform": "Transform"}
HANDLES = ("arslam_lm", "arslam_localizer", "arslam_slam")       # opaque: a pointer to one is a void*
CALLBACKS = {"arslam_allreduce_fn": "ALLREDUCE_FN", "arslam_iteration_callback": "ITER_CB"}
SCALARS = {"int": C.c_int, "double": C.c_double, "long": C.c_long, "unsigned": C.c_uint, "char": C.c_char,
           "unsigned char": C.c_ubyte, "unsigned long long": C.c_ulonglong, "size_t": C.c_size_t}
# (symbol, parameter index): the table's type where it is not the header's.  Exactly the two comm
# ids, unsigned char[128] in the header and c_char_p in the table because callers pass bytes.
SUBSTITUTIONS = {("arslam_comm_unique_id", 0): C.c_char_p, ("arslam_lm_set_comm", 3): C.c_char_p}


def _source(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _declarator(text):
    """'const double *cap' or 'int grid[2]' -> (base type, pointer depth, name, array length text or None)."""
    m = re.match(r"^(.*?)(\w+)\s*(?:\[([^\]]*)\])?$", re.sub(r"\bconst\b", " ", text).strip(), flags=re.S)
    return " ".join(m.group(1).replace("*", " ").split()), m.group(1).count("*"), m.group(2), m.group(3)


def _ctype(L, base, depth):
    if depth == 0:
        if base in MIRRORS:
            return getattr(L, MIRRORS[base])
        return getattr(L, CALLBACKS[base]) if base in CALLBACKS else SCALARS[base]
    if base == "char":
        t = C.c_char_p
    elif base == "void" or base in HANDLES:
        t = C.c_void_p
    else:
        t = C.POINTER(_ctype(L, base, 0))
    for _ in range(depth - 1):
        t = C.POINTER(t)
    return t


def _prototypes(L, header):
    """{symbol: (restype, [argtypes])} of every prototype of the header, in ctypes."""
    out = {}
    for ret, name, params in re.findall(r"^[ \t]*((?:\w+\s+)+\**)\s*(arslam_\w+)\s*\(([^()]*)\)\s*;", _source(header),
                                        flags=re.M):
        base, depth, _, _ = _declarator(ret + " _")
        args = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            pbase, pdepth, _, length = _declarator(p)
            args.append(_ctype(L, pbase, pdepth + (length is not None)))   # T x[N] is T*
        out[name] = (None if (base, depth) == ("void", 0) else _ctype(L, base, depth), args)
    return out


def _structs(L, header):
    """{struct name: [(field, ctypes type)]} of every typedef struct of the header."""
    src = _source(header)
    defines = {k: int(v) for k, v in re.findall(r"^#define\s+(\w+)\s+\(?(-?\d+)\)?\s*$", src, flags=re.M)}
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", src, flags=re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *rest = decl.split(",")
            base, depth, fname, length = _declarator(first)
            for d, f, n in [(depth, fname, length)] + [_declarator(r)[1:] for r in rest]:
                t = _ctype(L, base, d)
                fields.append((f, t if n is None else t * int(eval(n, {"__builtins__": {}}, defines))))
        out[name] = fields
    return out


@pytest.mark.parametrize("header", HEADERS)
def test_signature_table_matches_header(L, header):
    protos = _prototypes(L, header)
    assert sorted(protos) == _declared(header)          # the parser saw every declared symbol
    for name, (restype, argtypes) in protos.items():
        expected = [SUBSTITUTIONS.get((name, i), t) for i, t in enumerate(argtypes)]
        assert L.SIGNATURES[name] == expected, name
        assert L.RESTYPES.get(name, C.c_int) == restype, name
        fn = getattr(L.lib(), name)                     # and lib() applied the table
        assert list(fn.argtypes) == expected and fn.restype == restype, name


def test_signature_table_is_exactly_the_declared_symbols(L):
    declared = sorted(n for h in HEADERS for n in _declared(h))
    assert len(set(declared)) == len(declared)
    assert sorted(L.SIGNATURES) == declared and sorted(L.EXPORTS) == declared
    assert set(L.RESTYPES) <= set(L.SIGNATURES)
    assert set(SUBSTITUTIONS) <= {("arslam_comm_unique_id", 0), ("arslam_lm_set_comm", 3)} and len(SUBSTITUTIONS) <= 2
    for (name, i), t in SUBSTITUTIONS.items():          # each is the header's unsigned char* and nothing else
        proto = next(_prototypes(L, h)[name] for h in HEADERS if name in _declared(h))
        assert proto[1][i] == C.POINTER(C.c_ubyte) and t == C.c_char_p


@pytest.mark.parametrize("header", HEADERS)
def test_struct_mirrors_match_header(L, header):
    structs = _structs(L, header)
    assert set(structs) <= set(MIRRORS)                 # a new struct needs a mirror
    for name, fields in structs.items():
        assert list(getattr(L, MIRRORS[name])._fields_) == fields, name


def test_every_mirror_is_of_a_header_struct(L):
    assert sorted(n for h in HEADERS for n in _structs(L, h)) == sorted(MIRRORS)


def test_module_surface_is_unchanged(L):
    """Every name of ar_slam_amd.lm that was public, or that a test used, when lm.py became a package."""
    names = open(os.path.join(ROOT, "tests", "golden", "lm_surface.txt")).read().split()
    assert len(names) >= 95
    assert [n for n in names if not hasattr(L, n)] == []


def test_applying_the_table_tolerates_missing_symbols(L):
    class Fn:
        argtypes = restype = "untyped"

    class OlderBuild:       # a library that lacks some of the table's symbols, as a variant build under A/B may
        pass

    absent = {"arslam_lm_evaluate", "arslam_lm_covariance_lens", "arslam_debug_dag_tasks", "arslam_slam_destroy"}
    old = OlderBuild()
    for n in set(L.SIGNATURES) - absent:
        setattr(old, n, Fn())
    assert L.apply_signatures(old) is old
    for n in absent:
        assert not hasattr(old, n)
    for n in set(L.SIGNATURES) - absent:
        fn = getattr(old, n)
        assert fn.argtypes == L.SIGNATURES[n] and fn.restype == L.RESTYPES.get(n, C.c_int), n
    assert old.arslam_lm_destroy.restype is None and old.arslam_lm_version.restype == C.c_char_p


@pytest.mark.parametrize("header", HEADERS)
def test_library_exports_every_declared_symbol(L, header):
    lib = C.CDLL(L.library_path())
    names = _declared(header)
    assert names
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/{header} but not exported"
    for n in names:
        assert n in L.EXPORTS


def test_options_defaults_are_the_reference_settings(L):
    o = L.make_options()
    assert o.max_num_iterations == 50               # ar_slam_util.cpp:1004
    assert o.function_tolerance == 1e-6 and o.gradient_tolerance == 1e-10
    assert o.parameter_tolerance == 1e-8 and o.initial_trust_region_radius == 1e4
    assert o.min_lm_diagonal == 1e-6 and o.max_lm_diagonal == 1e32
    assert o.max_num_consecutive_invalid_steps == 5 and o.jacobi_scaling == 1
    with pytest.raises(AttributeError):
        L.make_options(no_such_option=1)


def test_summary_struct_matches_header(L):
    # ctypes mirror of arslam_lm_summary must be the size the library expects:
    # a mismatch would corrupt memory, so check the field order against the header
    src = open(os.path.join(ROOT, "include", "arslam_lm.h")).read()
    body = src[src.index("typedef struct {\n  int termination;"):src.index("} arslam_lm_summary;")]
    fields = re.findall(r"\b(\w+)(?:\[[^\]]*\])?\s*[;,]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    fields = [f for f in fields if f not in ("int", "double", "long")]
    ours = [f for f, _ in L.Summary._fields_]
    assert ours == fields


def test_problem_building_and_validation(L):
    prob = L.Problem()
    cam = np.array([900.0, 0.0, 0.0])
    caps = [np.zeros(6) for _ in range(2)]
    tags = [np.zeros(6) for _ in range(3)]
    prob.add_residual_block(np.zeros(8), cam, caps[0], tags[0])
    prob.add_residual_block(np.zeros(8), cam, caps[1], tags[2])
    assert prob.num_residual_blocks() == 2
    with pytest.raises(L.LMError):           # second camera block: unsupported
        prob.add_residual_block(np.zeros(8), np.zeros(3), caps[0], tags[0])
    with pytest.raises(L.LMError):           # capture reused as a tag
        prob.add_residual_block(np.zeros(8), cam, caps[0], caps[1])
    with pytest.raises(L.LMError):           # not part of the problem
        prob.set_parameter_block_constant(np.zeros(6))
    prob.set_parameter_block_constant(tags[0])
    prob.reset()
    assert prob.num_residual_blocks() == 0
    with pytest.raises(TypeError):
        prob.add_residual_block(np.zeros(8), cam, np.zeros(5), tags[0])


def test_solve_without_gpu_fails_loudly(L):
    if L.device_count() > 0:
        pytest.skip("a GPU is present")
    from ar_slam_amd import synth
    g = synth.config_graph("tiny")
    with pytest.raises(L.LMError):
        L.solve_graph(g)


def test_empty_problem_converges_immediately(L):
    s = L.Problem().solve()
    assert s["termination"] == "CONVERGENCE" and s["num_linear_solves"] == 0


def test_set_and_get_options_roundtrip(L):
    """Per-solve options (ArSlamSolver::optimize builds Solver::Options per call, ar_slam_util.cpp:1003-1012)."""
    prob = L.Problem()
    prob.set_options(max_num_iterations=7, minimizer_progress_to_stdout=1, function_tolerance=1e-9)
    o = prob.get_options()
    assert o.max_num_iterations == 7 and o.minimizer_progress_to_stdout == 1
    assert o.function_tolerance == 1e-9
    with pytest.raises(L.LMError):
        prob.set_options(max_num_iterations=-1)
    with pytest.raises(L.LMError):
        prob.set_options(elimination=5)
    assert prob.get_options().max_num_iterations == 7   # a rejected call leaves the options unchanged
