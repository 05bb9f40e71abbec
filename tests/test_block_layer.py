"""not-gpu: the block layer linalg/_block.py stands below every eigensolver driver -- who imports whom (read from the
syntax trees), the names the drivers re-export, and the values of what moved there."""
import ast
import pathlib
import pytest
import torch
from xitorch_amd.linalg import _block, host_eig, native_eig, native_eig_herm, native_chebfsi, native_lobpcg

LINALG = pathlib.Path(_block.__file__).parent


def _imports(module, nested_only=False):
    """[(module name, imported names)] of a module's import statements; nested_only: those inside a function"""
    tree = ast.parse((LINALG / (module + ".py")).read_text())
    top = set(map(id, tree.body))
    found = []
    for node in ast.walk(tree):
        if nested_only and id(node) in top:
            continue
        if isinstance(node, ast.ImportFrom):
            found.append((node.module or "", [a.name for a in node.names]))
        elif isinstance(node, ast.Import):
            found.extend((a.name, []) for a in node.names)
    return found


def _names_drivers(entry):
    """does the import (module, names) reach a native_* / host_* module of the package?"""
    mod, names = entry
    parts = mod.split(".") + (names if mod.endswith("linalg") else [])
    return any(p.startswith(("native_", "host_")) for p in parts)


def test_block_layer_imports_no_driver():
    reaching = [e for e in _imports("_block") if _names_drivers(e)]
    assert reaching == []
    assert any(mod == "xitorch_amd.linalg._panel" for mod, _ in _imports("_block"))


def test_host_twin_names_native_eig_for_exacteig_only():
    entries = [e for e in _imports("host_eig") if "native_" in e[0] or any(n.startswith("native_") for n in e[1])]
    assert entries and all(e == ("xitorch_amd.linalg.native_eig", ["exacteig"]) for e in entries), entries
    assert ("xitorch_amd.linalg._block", ["_initial_block", "_shard_of_global_batch", "_shift_rel", "GUARD_BAD",
                                          "GUARD_MAX_REDO"]) in _imports("host_eig")


@pytest.mark.parametrize("module", ["native_chebfsi", "native_lobpcg"])
def test_block_drivers_import_the_davidson_drivers_for_exacteig_only(module):
    nested = [e for e in _imports(module, nested_only=True) if _names_drivers(e)]
    assert nested == [("xitorch_amd.linalg.native_eig", ["exacteig"])], nested
    everywhere = [e for e in _imports(module) if "native_eig" in e[0] or "native_eig" in " ".join(e[1])]
    assert everywhere == nested


def test_reexported_names_are_the_block_layer_objects():
    for name in ("native_partial_eigh", "_native_dense_ok", "take_eigpairs", "GUARD_GOOD", "GUARD_BAD",
                 "GUARD_MAX_REDO", "EXACTEIG_NATIVE_MAX_P", "K3G_MAX_K", "_initial_block", "_preconditioner"):
        assert getattr(native_eig, name) is getattr(_block, name), name
    for name in ("herm_partial_eigh", "_shift_rel"):
        assert getattr(native_eig_herm, name) is getattr(_block, name), name
    assert host_eig.GUARD_BAD is _block.GUARD_BAD and host_eig._shift_rel is _block._shift_rel
    assert native_chebfsi.GUARD_BAD is _block.GUARD_BAD and native_lobpcg.GUARD_BAD is _block.GUARD_BAD
    # exacteig looks the predicate up in native_eig's namespace: that is where test_gpu_exacteig patches it
    assert native_eig.exacteig.__globals__ is vars(native_eig)


def test_values_that_moved():
    assert _block.GUARD_GOOD == {torch.float64: 1e-10, torch.float32: 5e-5}
    assert _block.GUARD_BAD == {torch.float64: 1e-8, torch.float32: 5e-4}
    assert _block.GUARD_MAX_REDO == 3
    shift = {(torch.float64, 257, 5): 1.605937605120289e-12, (torch.float64, 1037, 6): 7.649880728877179e-12,
             (torch.float64, 16384, 32): 6.415739051135461e-10, (torch.float32, 257, 5): 0.0008621811866760254,
             (torch.float32, 1037, 6): 0.001, (torch.float32, 16384, 32): 0.001}
    for (rdtype, N, q), value in shift.items():
        assert _block._shift_rel(N, q, rdtype) == value, (rdtype, N, q)
    lam = torch.arange(5.0)
    U = torch.arange(20.0).reshape(4, 5)
    lo, Ulo = _block.take_eigpairs(lam, U, 2, "lowest")
    up, Uup = _block.take_eigpairs(lam, U, 2, "uppest")
    assert lo.tolist() == [0.0, 1.0] and up.tolist() == [3.0, 4.0]
    assert torch.equal(Ulo, U[:, :2]) and torch.equal(Uup, U[:, 3:])
