"""CPU guard of the instance ledger: the kernels tests/instance_ledger.json
records, plus the allow-list of tests/instance_matrix.py, are exactly the project
kernels of the built library (tests/kernel_inventory.py).  An instance added,
removed or renamed without a case that launches it fails here, before any GPU
run; the ledger itself is checked on the GPU (tests/test_gpu_instance_matrix.py)."""
import pytest

import instance_matrix as M
import kernel_inventory as K


@pytest.fixture(scope="module")
def inventory():
    try:
        return set(K.project_kernels())
    except K.InventoryError as e:
        pytest.fail(str(e))


def test_ledger_plus_allow_list_is_the_inventory(inventory):
    ledger = M.load_ledger()
    covered = set(ledger) | set(M.ALLOW)
    missing, gone = sorted(inventory - covered), sorted(covered - inventory)
    msg = []
    if missing:
        msg.append(f"{len(missing)} compiled instances have no case (add one to tests/instance_matrix.py and "
                   "regenerate the ledger with `python tests/instance_matrix.py --write-ledger`):\n  " + "\n  ".join(missing))
    if gone:
        msg.append(f"{len(gone)} ledger / allow-list entries are no longer compiled:\n  " + "\n  ".join(gone))
    assert not msg, "\n".join(msg)
    both = sorted(set(ledger) & set(M.ALLOW))
    assert not both, f"allow-listed as unreachable, yet in the ledger: {both}"


def test_ledger_names_the_matrix_cases():
    ids = set(M.CASE_IDS)
    for kernel, cases in M.load_ledger().items():
        assert K.is_project_kernel(kernel), kernel
        assert cases and cases == sorted(set(cases)), kernel
        assert set(cases) <= ids, (kernel, sorted(set(cases) - ids))
    for kernel, reason in M.ALLOW.items():
        assert isinstance(reason, str) and ":" in reason, f"{kernel}: the reason cites file:line"


def test_inventory_reads_symbols_of_every_code_object(inventory):
    """The library's own kernels outnumber 200 and rocprim's are kept out."""
    assert len(inventory) > 200
    assert not any("rocprim" in k or "__amd_rocclr" in k for k in inventory)
