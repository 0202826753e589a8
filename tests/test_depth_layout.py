"""The layout of the depth leg's Python modules: depth_compose <- depth_routes <- depth_pro <- depth, imports in that one direction and at module top; the
rewrites of a module's ``forward`` live in depth_routes.py / depth_pro.py, not in DepthPipe; depth.py still exports every name that tests, tools and bench.py
import from it.  Host only: ast and two short child interpreters."""
import ast
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "visiondepth3d_amd")
MODULES = ("depth_compose", "depth_routes", "depth_pro", "depth")
# every name that tests/, tools/ and bench.py take from visiondepth3d_amd.depth (from-imports and attributes of the module)
REEXPORTS = ("CONV_X2_MIN_TILES", "DepthPipe", "HEAD_CONV2_GATHER_BUILT", "HEAD_CONV2_GATHER_ROUTED", "HEAD_UPCONV_BUILT", "IMAGENET_MEAN", "IMAGENET_STD", "MODEL_ZOO",
             "PROCESSORS", "_BitPrefix", "_PerVersion", "_SWITCHES", "_switch", "bit_prefix_plan", "bit_standardized_weight", "build_config",
             "conv_transpose_gemm_weight", "depth_to_u8", "dpt_resize_target", "head_conv2_compose", "head_upconv_compose", "im2col_gemm_weight", "neck_poly_compose",
             "neck_poly_offsets", "patch_embedding_gemm_weight", "patch_embedding_rows", "same_padding", "synthetic_weights_")


def _tree(module):
    with open(os.path.join(PKG, module + ".py")) as f:
        return ast.parse(f.read())


def _child(code):
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)


def test_depth_compose_imports_neither_transformers_nor_the_renderer():
    r = _child("import sys, visiondepth3d_amd.depth_compose\n"
               "print([m for m in ('transformers', 'visiondepth3d_amd.render_3d', 'visiondepth3d_amd._lib') if m in sys.modules])")
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "[]"


def test_depth_pro_imports_on_its_own():
    r = _child("import visiondepth3d_amd.depth_pro as P\nprint(P.encoders_scope.__name__, P.EncoderRoutes.__name__, P.DecoderRoutes.__name__)")
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["encoders_scope", "EncoderRoutes", "DecoderRoutes"]


@pytest.mark.parametrize("module", MODULES)
def test_no_function_imports_one_of_the_four_modules(module):
    """The import direction is visible at module top: no function body holds a relative import of depth, depth_pro, depth_routes or depth_compose."""
    found = []
    for fn in ast.walk(_tree(module)):
        if not isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda)):
            continue
        for n in ast.walk(fn):
            if isinstance(n, ast.ImportFrom) and n.level >= 1:
                hit = [n.module] if n.module in MODULES else [a.name for a in n.names if n.module is None and a.name in MODULES]
                found += [(getattr(fn, "name", "lambda"), n.lineno, h) for h in hit]
    assert not found, found


def test_the_import_direction_at_module_top():
    """A module imports only those to its left in depth_compose <- depth_routes <- depth_pro <- depth."""
    for i, module in enumerate(MODULES):
        for n in ast.walk(_tree(module)):
            if isinstance(n, ast.ImportFrom) and n.level >= 1:
                for name in ([n.module] if n.module else [a.name for a in n.names]):
                    assert name not in MODULES[i:], (module, n.lineno, name)


def test_depth_py_assigns_no_forward():
    hits = [n.lineno for n in ast.walk(_tree("depth")) if isinstance(n, (ast.Assign, ast.AugAssign, ast.AnnAssign))
            for t in (n.targets if isinstance(n, ast.Assign) else [n.target]) for a in ast.walk(t) if isinstance(a, ast.Attribute) and a.attr == "forward"]
    assert not hits, hits


def test_depth_pipe_lost_the_model_surgery():
    gone = ("_patch_da_reassemble", "_self_contained_resize", "_self_contained_resize_run", "_self_contained_reassemble", "_patch_patch_embedding",
            "_patch_dpt_vit_reassemble_head", "_patch_hybrid_embeddings", "_depth_pro_encoders_scope", "_route_depth_pro_encoders")
    cls = next(n for n in _tree("depth").body if isinstance(n, ast.ClassDef) and n.name == "DepthPipe")
    methods = {n.name for n in cls.body if isinstance(n, ast.FunctionDef)}
    assert not methods & set(gone), methods & set(gone)
    assert {"_split_scope", "_rewrite_dpt_vit", "_patch_dpt_upsampling"} <= methods   # thin, and called by the host tests


def test_depth_reexports_what_tests_tools_and_bench_import():
    from visiondepth3d_amd import depth
    missing = [n for n in REEXPORTS if not hasattr(depth, n)]
    assert not missing, missing
