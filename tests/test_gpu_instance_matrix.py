"""Every compiled kernel instance under a comparison (tests/instance_matrix.py).

1. Parity: each case of the matrix against its reference, in this process.
2. The ledger: the matrix once more as a fresh child process under rocprofv3's
   kernel trace.  From the trace: every project kernel of the built library
   (tests/kernel_inventory.py) is launched by some case, bar the allow-list, and
   the map from kernel to the cases that launch it is the committed
   tests/instance_ledger.json, so that a ladder that moves a configuration onto
   another instance shows as a diff.  Regenerate the ledger with
   `python tests/instance_matrix.py --write-ledger` on the GPU.
"""
import json

import pytest

import instance_matrix as M
import kernel_inventory as K

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def no_spt_environment(monkeypatch):
    for k in M.config_variables():
        monkeypatch.delenv(k)


@pytest.fixture(scope="module", autouse=True)
def drop_cached_scenes():
    yield
    M._scenes.clear()


@pytest.mark.parametrize("case", M.CASES, ids=M.CASE_IDS)
def test_case_equals_its_reference(case):
    M.verify(case, M.run_case(case))


@pytest.fixture(scope="module")
def traced(tmp_path_factory):
    """The traced child, started once.  Nothing is raised here: the tests below fail on what it left."""
    tmp = str(tmp_path_factory.mktemp("instance_trace"))
    status, tail, seconds = M.traced_run(tmp)
    out = dict(status=status, tail=tail, seconds=seconds, ledger=None, outside=None, error=None)
    print(f"traced child: exit {status} after {seconds:.1f} s (limit {M.TRACE_LIMIT_S} s)")
    if status == 0:
        try:
            out["ledger"], out["outside"] = M.ledger_from_trace(tmp)
        except (AssertionError, OSError, KeyError, ValueError) as e:
            out["error"] = f"{type(e).__name__}: {e}"
    return out


def need_ledger(traced):
    assert traced["status"] is not None, f"rocprofv3 could not be started: {traced['tail']}"
    assert traced["status"] not in (124, 137), f"the traced child ran into its {M.TRACE_LIMIT_S} s limit:\n{traced['tail']}"
    assert traced["status"] == 0, f"the traced child exited {traced['status']}:\n{traced['tail']}"
    assert traced["error"] is None, traced["error"]
    return traced["ledger"]


def test_traced_child_exits_clean(traced):
    need_ledger(traced)
    assert not traced["outside"], f"project kernels launched outside every case: {traced['outside']}"


def test_every_instance_is_launched(traced):
    launched = set(need_ledger(traced))
    inventory = set(K.project_kernels())
    never = sorted(inventory - launched - set(M.ALLOW))
    assert not never, f"{len(never)} of {len(inventory)} instances never launched:\n" + "\n".join(never)
    stale = sorted(set(M.ALLOW) & launched)
    assert not stale, f"allow-listed as unreachable, yet launched: {stale}"
    unknown = sorted(launched - inventory)
    assert not unknown, f"launched, but not in the library's inventory: {unknown}"


def test_ledger_is_reproduced(traced):
    got, want = need_ledger(traced), M.load_ledger()
    moved = []
    for k in sorted(set(got) | set(want)):
        a, b = set(got.get(k, ())), set(want.get(k, ()))
        if a != b:
            moved.append(f"{k}\n    no longer: {sorted(b - a)}\n    new: {sorted(a - b)}")
    assert not moved, "the run launches other instances than tests/instance_ledger.json records:\n" + "\n".join(moved)
    assert json.dumps(got, sort_keys=True) == json.dumps(want, sort_keys=True)
