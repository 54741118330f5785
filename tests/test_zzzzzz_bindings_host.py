"""CPU tests of the Python binding glue: the five ctypes bindings (_lib, _lib_ext, _lib_moe, _lib_moe_data, _lib_moe_gemm) load through
the one loader of _lib.py -- every exported symbol declared from the binding's prototype table, one library object per process, and a
stale, incomplete or missing library refused with NNopLibraryMissing and the message that says how to rebuild -- and the operator
modules share the call plumbing of _common.py instead of carrying copies.

The file name sorts behind every existing test file on purpose, as tests/test_residual_addnorm_gpu.py explains."""
import pytest

REBUILD = "rebuild with `make -C nnop.jl_amd/csrc -j8`"
# binding module, the name of its version constant, the label of its version in the message
BINDINGS = [("_lib", "ABI_VERSION", "ABI version"),
            ("_lib_ext", "EXT_ABI_VERSION", "ext-ABI version"),
            ("_lib_moe", "MOE_ABI_VERSION", "moe-ABI version"),
            ("_lib_moe_data", "MOE_DATA_ABI_VERSION", "moe-data-ABI version"),
            ("_lib_moe_gemm", "MOE_GEMM_ABI_VERSION", "moe-gemm-ABI version")]
OPERATORS = ("attention", "rope", "softmax", "norms", "activations", "losses", "qknorm", "moe", "moe_data", "moe_gemm")
binding = pytest.mark.parametrize("mod,const,label", BINDINGS, ids=[b[0] for b in BINDINGS])


@binding
def test_load_declares_every_exported_symbol(pkg, mod, const, label):
    M = getattr(pkg, mod)
    lib = M.load()
    assert M.EXPORTED_SYMBOLS == tuple(M.PROTOTYPES)
    for name in M.EXPORTED_SYMBOLS:
        restype, argtypes = M.PROTOTYPES[name]
        fn = getattr(lib, name)
        assert fn.restype is restype, name
        assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name      # None: never declared


@binding
def test_second_load_returns_the_same_object(pkg, mod, const, label):
    M = getattr(pkg, mod)
    assert M.load() is M.load() is M._lib


@binding
def test_stale_incomplete_or_missing_library_is_refused(pkg, monkeypatch, mod, const, label):
    M = getattr(pkg, mod)
    version = getattr(M, const)
    monkeypatch.setattr(M, "_lib", None)
    monkeypatch.setattr(M, const, version + 1)
    with pytest.raises(pkg._lib.NNopLibraryMissing) as e:
        M.load()
    assert str(e.value) == f"{M.LIB_PATH} has {label} {version}, this binding needs {version + 1}: {REBUILD}"
    monkeypatch.setattr(M, const, version)
    monkeypatch.setattr(M, "EXPORTED_SYMBOLS", M.EXPORTED_SYMBOLS + ("nnop_not_there",))
    with pytest.raises(pkg._lib.NNopLibraryMissing) as e:
        M.load()
    assert str(e.value) == f"{M.LIB_PATH} does not export nnop_not_there: {REBUILD}"
    monkeypatch.setattr(M, "LIB_PATH", "/nonexistent/libnnop.so")
    with pytest.raises(pkg._lib.NNopLibraryMissing) as e:
        M.load()
    assert str(e.value) == ("/nonexistent/libnnop.so not found: build it with `make -C nnop.jl_amd/csrc -j8` "
                            "(or __graft_entry__.build()).  There is no CPU or PyTorch fallback.")
    assert M._lib is None                        # a refused load leaves nothing behind


def test_the_error_type_is_one_class(pkg):
    assert pkg.NNopError is pkg.attention.NNopError is pkg._common.NNopError
    assert issubclass(pkg.NNopError, RuntimeError)


@pytest.mark.parametrize("op", OPERATORS)
def test_operator_modules_share_the_call_plumbing(pkg, op):
    """what a module has of the shared helpers is _common's object, not a copy (a module that never needs one does not carry it)"""
    module, common = getattr(pkg, op), pkg._common
    assert module.NNopError is common.NNopError and module._DTYPES is common._DTYPES
    for name in ("_ptr", "_stream", "_on_device", "_raise", "_launch", "_dtype_name"):
        assert vars(module).get(name, getattr(common, name)) is getattr(common, name), f"{op}.{name}"
    assert any(name in vars(module) for name in ("_ptr", "_launch"))           # ... and it does reach the library through them
