"""Which kernels a call launched: the library's exact launch record (``pcc_profile_names`` through ``_lib.profile()``)
around one function call.  A test that names a kernel variant -- forced through ``_lib.tuning`` or chosen by a size next to
a switch point -- asserts with these helpers that this variant, and no sibling of its family, is what executed; the
expected name comes from the rule restated in the op's ``tests/*_reference.py``, never from the library."""


def ran(fn):
    """``(fn(), {exact profile name: launches})`` of everything the library launched while ``fn`` ran."""
    from pointcloudcounterfactual_amd import _lib

    with _lib.profile() as read:
        result = fn()
        names = read.exact()
    return result, names


def family(names, *prefixes):
    """The part of a launch record whose names begin with one of ``prefixes`` (the siblings of one switch)."""
    return {k: v for k, v in names.items() if k.startswith(prefixes)}


def assert_only(names, expected, *prefixes):
    """Of the kernels whose names begin with ``prefixes``, exactly those of ``expected`` (a name or a collection of names)
    ran: each at least once, and no sibling.  Without ``prefixes`` the whole record is compared."""
    expected = {expected} if isinstance(expected, str) else set(expected)
    got = family(names, *prefixes) if prefixes else names
    assert set(got) == expected, f'expected {sorted(expected)}, the launch record has {got} (all launches: {names})'


def ran_only(fn, expected, *prefixes):
    """``fn()`` once ``assert_only`` holds for what it launched."""
    result, names = ran(fn)
    assert_only(names, expected, *prefixes)
    return result


# ---- the census (tests/kernel_census.py): a test the table names for a kernel proves, on every run, that it ran ----
import pytest  # noqa: E402


def _census_needs(nodeid, original):
    """The kernels tests/kernel_census.py maps to this test: to the function (every case must run them) or to this case."""
    from tests.kernel_census import CENSUS

    path, _, case = nodeid.partition('::')
    function = f'{path}::{original}'
    return sorted(k for k, v in CENSUS.items() if v is not None and v in (function, f'{path}::{case}'))


@pytest.fixture(autouse=True)
def census_proof(request):
    """Imported by the GPU test modules the census names (``from tests.which_ran import census_proof``).  For a test the
    census lists, the whole test runs with the launch profile on, and at its end every kernel the census maps to it must be
    in the exact launch record; for any other test this does nothing.  The record survives the profile scopes the test opens
    itself (``ran``, ``_lib.profile()``, ``pcc_profile_enable``): it is read before each of them clears it.  Side effect,
    for a listed test only: ``pcc_profile_enable`` and ``pcc_profile_reset`` of ``_lib.lib`` are wrapped while it runs, and a
    disable becomes ``enable(1)`` so that the test's own record goes on -- such a test cannot observe profiling off (no
    listed test reads the profile after disabling it)."""
    needs = _census_needs(request.node.nodeid, getattr(request.node, 'originalname', None) or request.node.name)
    if not needs:
        yield
        return
    import ctypes

    import torch

    from pointcloudcounterfactual_amd import _lib

    L, seen = _lib.lib, set()
    enable, reset, names = L.pcc_profile_enable, L.pcc_profile_reset, L.pcc_profile_names

    def snapshot():
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(names(None, 0))
        names(buf, len(buf))
        seen.update(line.split('\t')[0] for line in buf.value.decode().splitlines())

    def enable_keeping(on):
        snapshot()
        enable(on if on else 1)  # (a scope that ends inside the test leaves the test's own record running)

    def reset_keeping():
        snapshot()
        reset()

    L.pcc_profile_enable, L.pcc_profile_reset = enable_keeping, reset_keeping
    failed_before = request.session.testsfailed
    enable(1)
    try:
        yield
        snapshot()
    finally:
        L.pcc_profile_enable, L.pcc_profile_reset = enable, reset
        enable(0)
        reset()
    if request.session.testsfailed > failed_before:
        return  # (the test itself failed, perhaps before it got to the kernel: one report is enough)
    missing = [k for k in needs if k not in seen]
    assert not missing, f'the census names this test for kernels it did not launch: {missing}'
