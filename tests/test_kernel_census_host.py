"""Host tests of the kernel census (tests/kernel_census.py): every kernel name the library can record in its launch
profile is in the table, mapped to a GPU test that exists and carries the proof fixture, or listed as unproven with a
reason -- at most MAX_UNPROVEN of them.  Runs without a GPU: it reads the sources."""

import glob
import os
import re

from tests.kernel_census import CENSUS, MAX_UNPROVEN, UNPROVEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pointcloudcounterfactual_amd', 'csrc')
LITERAL = re.compile(r'"([A-Za-z0-9_]*_kernel[^"\n]*)"')
# "..._kernel..." literals of the sources that are no profile names
NOT_PROFILE_NAMES = {
    'scatter_bwd_kernel<...>',  # graph_ops.hip, a comment: the placeholder for the three scatter_bwd_kernel<...> names
    'am_sort_kernel',           # cloud_sort.hip, a comment: the prefix under which the five am_sort_kernel<slots> names are counted
}


def kernel_literals(csrc=CSRC):
    """The ``"..._kernel..."`` string literals of ``csrc/*.hip`` and ``*.hpp``."""
    found = set()
    for path in sorted(glob.glob(os.path.join(csrc, '*.hip')) + glob.glob(os.path.join(csrc, '*.hpp'))):
        with open(path) as f:
            found |= set(LITERAL.findall(f.read()))
    return found


def uncatalogued(csrc=CSRC):
    return sorted(kernel_literals(csrc) - set(CENSUS) - NOT_PROFILE_NAMES)


def test_every_kernel_name_of_the_sources_is_in_the_census():
    assert len(kernel_literals()) > 200  # (the expression still finds them)
    assert uncatalogued() == [], 'kernel names without a census entry (tests/kernel_census.py)'
    assert NOT_PROFILE_NAMES <= kernel_literals() and not NOT_PROFILE_NAMES & set(CENSUS)


def test_the_census_names_no_kernel_the_sources_have_dropped():
    assert sorted(set(CENSUS) - kernel_literals()) == []


def test_every_census_value_names_an_existing_test_that_carries_the_proof():
    sources = {}
    for kernel, where in CENSUS.items():
        if where is None:
            continue
        path, _, test = where.partition('::')
        function = test.partition('[')[0]
        assert path.startswith('tests/test_') and function.startswith('test_'), (kernel, where)
        if path not in sources:
            with open(os.path.join(ROOT, path)) as f:
                sources[path] = f.read()
        assert re.search(rf'^def {re.escape(function)}\(', sources[path], re.M), (kernel, where)
        # the module imports the fixture that asserts, in this very test, that the kernel ran (tests/which_ran.py)
        assert re.search(r'^from tests\.which_ran import .*\bcensus_proof\b', sources[path], re.M), (kernel, path)
        assert re.search(r'^pytestmark = pytest\.mark\.gpu|^@pytest\.mark\.gpu', sources[path], re.M), path


def test_unproven_kernels_carry_a_reason_and_stay_under_the_cap():
    unproven = {kernel for kernel, where in CENSUS.items() if where is None}
    assert unproven == set(UNPROVEN) and all(len(reason) > 20 for reason in UNPROVEN.values())
    assert len(unproven) <= MAX_UNPROVEN == 8


def test_the_literal_search_notices_a_new_name(tmp_path):
    (tmp_path / 'new.hip').write_text('void f() { pcc::ProfScope prof("brand_new_kernel<7>", st); }\n')
    assert kernel_literals(str(tmp_path)) == {'brand_new_kernel<7>'} and uncatalogued(str(tmp_path)) == ['brand_new_kernel<7>']
