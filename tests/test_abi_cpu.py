"""CPU-side checks of the drop-in boundary: the C-ABI library builds, loads without a GPU and exports
every symbol include/radsearch.h declares; the ctypes binding covers all of them; no compute calls."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from radiation_ppo_amd import build
    build.build(verbose=False)
    from radiation_ppo_amd import _lib
    return _lib.load()


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "radsearch.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rs_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported(lib):
    names = _declared_symbols()
    assert "rs_step" in names and "rs_reset" in names and "rs_gae" in names and "rs_create" in names
    assert "rs_cnn_trunk_forward_grid" in names and "rs_cnn_trunk_slab_rows" in names        # the host-only grid queries of the CNN trunk
    for n in names:
        assert hasattr(lib, n), f"librs_hip.so does not export {n}"


def test_binding_covers_header(lib):
    from radiation_ppo_amd import _lib
    bound = {s[0] for s in _lib.SYMBOLS}
    assert bound == set(_declared_symbols())


def test_config_validation_and_errors(lib):
    from radiation_ppo_amd import _lib
    good = _lib.RsConfig(num_envs=4, num_agents=1, obstruction_count=0, enforce_grid_boundaries=1,
                         bbox=(0, 0, 2700, 2700), observation_area=(200, 500), falloff=0, geom_group_size=1,
                         seed=2, env_id_base=0)
    assert lib.rs_state_bytes(ctypes.byref(good)) > 0
    for field, bad in (("num_envs", 0), ("num_agents", 9), ("obstruction_count", 8), ("obstruction_count", -2),
                       ("geom_group_size", 0)):
        cfg = _lib.RsConfig.from_buffer_copy(good)
        setattr(cfg, field, bad)
        assert lib.rs_state_bytes(ctypes.byref(cfg)) == 0
    h = ctypes.c_void_p()
    assert lib.rs_create(ctypes.byref(good), None, 0, None, ctypes.byref(h)) == 1        # RS_ERR_INVALID_ARG
    assert lib.rs_strerror(0) == b"ok" and b"workspace" in lib.rs_strerror(3)
    assert lib.rs_step(None, None, None, None, None, None, None, None) == 1


def test_product_does_not_import_oracle():
    """The oracle is test infrastructure: nothing under radiation_ppo_amd/ may import or execute it."""
    pkg = os.path.join(ROOT, "radiation_ppo_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp")):
                txt = open(os.path.join(d, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", txt, flags=re.M), (d, f)
                assert "oracle/" not in txt and "radsearch_oracle" not in txt, (d, f)


def test_env_requires_gpu_and_fails_loudly():
    import torch
    from radiation_ppo_amd.envs import RadSearchVec
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError):
        RadSearchVec(4, device="cpu")
