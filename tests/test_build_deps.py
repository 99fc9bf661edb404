"""gymnasium_amd/csrc/build.py finds a unit's dependencies itself: the transitive closure of its `#include "..."` lines (build.includes), which
_stale compares with the object file.  CPU only; nothing in the tree is touched (the staleness test works on copies)."""
import functools
import os
import shutil

import pytest

from gymnasium_amd.csrc import build as B

ROOT = os.path.normpath(os.path.join(B.HERE, "..", ".."))


@functools.lru_cache(maxsize=None)
def closure(unit):  # (generated/mjx_models.h is a committed file: nothing to generate first)
    return {os.path.relpath(f, B.HERE) for f in B.includes(os.path.join(B.HERE, unit))}


def test_closure_of_engine():
    deps = closure("engine.hip")
    for name in ("engine_types.h", os.path.join("..", "..", "include", "mi355env.h")):
        assert name in deps, name
    assert not any(f.endswith(".hip") for f in deps)
    # the C ABI holds no environment family's kernels: those are mujoco.hip's, tabular.hip's and classic.hip's
    for name in ("tabular_kernels.h", "mj_glue_kernels.h", "mj_wrapped_kernels.h", "mjx_physics.h", "mjx_coop.h", "mjx_core.h",
                 os.path.join("generated", "mjx_models.h"), "classic_kernels.h", "lane_step.h"):
        assert name not in deps, name


def test_closure_of_mujoco():
    deps = closure("mujoco.hip")
    for name in ("mj_glue_kernels.h", "mj_wrapped_kernels.h", "mjx_physics.h", "mj_lane_launch.h", os.path.join("generated", "mjx_models.h")):
        assert name in deps, name
    assert "tabular_kernels.h" not in deps and "classic_kernels.h" not in deps and not any(f.endswith(".hip") for f in deps)


def test_closure_of_tabular():
    deps = closure("tabular.hip")
    assert "tabular_kernels.h" in deps and "classic_kernels.h" not in deps
    assert not any(os.path.basename(f).startswith(("mjx_", "mj_")) for f in deps), deps


def test_closure_of_classic():
    deps = closure("classic.hip")
    assert "sincos_table.h" in deps and "envs_classic.h" in deps
    assert "classic_kernels.h" in deps and "lane_step.h" in deps
    assert not any(os.path.basename(f).startswith("mjx_") for f in deps), deps
    assert "mj_glue_kernels.h" not in deps and "tabular_kernels.h" not in deps and not any(f.endswith(".hip") for f in deps)


def test_closure_of_mjx_model():
    deps = closure("mjx_model.hip")
    assert "mj_glue_kernels.h" in deps and "engine_types.h" in deps and os.path.join("generated", "mjx_models.h") in deps
    assert "wrappers_internal.h" not in deps and "mjx_physics.h" not in deps and not any(f.endswith(".hip") for f in deps)


@pytest.mark.parametrize("unit", B.SOURCES)
def test_no_unit_includes_a_unit(unit):
    assert not any(f.endswith(".hip") for f in closure(unit))


@pytest.fixture(scope="module")
def tree_copy(tmp_path_factory):
    """csrc's sources and include/ copied once"""
    B.generate_models()
    top = tmp_path_factory.mktemp("tree")
    shutil.copytree(B.HERE, top / "gymnasium_amd" / "csrc", ignore=shutil.ignore_patterns("*.o", "*.so", "__pycache__"))
    shutil.copytree(os.path.join(ROOT, "include"), top / "include")
    return top


@pytest.fixture
def copied_tree(tree_copy, monkeypatch):
    """every copied file at one old mtime, an 'object file' per unit a little newer; build.HERE points at the copy"""
    here = tree_copy / "gymnasium_amd" / "csrc"
    for folder, _, files in os.walk(tree_copy):
        for f in files:
            os.utime(os.path.join(folder, f), (1_000_000, 1_000_000))
    for unit in B.SOURCES:
        obj = here / (os.path.splitext(unit)[0] + ".o")
        obj.write_bytes(b"")
        os.utime(obj, (1_000_100, 1_000_100))
    monkeypatch.setattr(B, "HERE", str(here))
    return here


def stale_units(here):
    return {unit for unit in B.SOURCES if B._stale(str(here / (os.path.splitext(unit)[0] + ".o")), unit)}


@pytest.mark.parametrize("header", ["mj_glue_kernels.h", "lane_common.h", "wrappers_internal.h", "pcg64_dev.h", "action_mask_internal.h",
                                    "classic_kernels.h", "lane_step.h", "tabular_kernels.h", "candidate_lane.h",
                                    os.path.join("generated", "mjx_models.h"), os.path.join("..", "..", "include", "mi355env.h")])
def test_touching_a_header_makes_its_includers_stale(copied_tree, header):
    os.utime(os.path.join(copied_tree, header), (1_000_200, 1_000_200))
    expected = {unit for unit in B.SOURCES if os.path.normpath(header) in closure(unit)}  # (closure() reads the tree itself: computed once per unit)
    assert expected, header
    assert stale_units(copied_tree) == expected
    if header == "mj_glue_kernels.h":
        assert {"mujoco.hip", "mjx_model.hip", "mjx_mass_model.hip"} <= expected and "engine.hip" not in expected
    if header == "lane_common.h":
        assert {"engine.hip", "mjx_model.hip"} <= expected
    if header == "wrappers_internal.h":
        assert {"wrappers.hip"} <= expected and "mjx_model.hip" not in expected
    if header == "action_mask_internal.h":
        assert {"engine.hip", "action_mask.hip"} <= expected
    if header in ("classic_kernels.h", "lane_step.h"):
        assert "classic.hip" in expected and "engine.hip" not in expected
    if header == "tabular_kernels.h":
        assert expected == {"tabular.hip"}
    if header == "candidate_lane.h":
        assert expected == {"lookahead.hip", "lookahead_policy.hip"}


def test_touching_a_unit_or_the_build_script(copied_tree):
    assert stale_units(copied_tree) == set()
    os.utime(copied_tree / "classic.hip", (1_000_200, 1_000_200))
    assert stale_units(copied_tree) == {"classic.hip"}
    os.utime(copied_tree / "mjx_model.hip", (1_000_250, 1_000_250))
    assert stale_units(copied_tree) == {"classic.hip", "mjx_model.hip"}
    os.utime(copied_tree / "build.py", (1_000_300, 1_000_300))
    assert stale_units(copied_tree) == set(B.SOURCES)
