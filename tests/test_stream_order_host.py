"""tests/stream_order.py without a device: the stream suite runs every computing symbol of the C ABI, its ``WAITS`` table
names symbols that exist, and a static companion for the launch sites no shape of the suite reaches.

The static check reads the library's sources: every ``hipLaunchKernelGGL``, ``hipMemsetAsync`` and ``hipMemcpyAsync`` must
name a stream, and the name must not be the literal ``0``, ``nullptr`` or ``NULL``; a ``<<< >>>`` launch must carry all four
configuration arguments.  This is weaker than running the launch: it sees the text of the argument, not its value -- a variable
that holds the wrong stream, or another call's, passes.  It is there for the instantiations and error paths the running suite
cannot select."""

import glob
import os
import re

from tests import stream_order as S
from tests import unaligned_views as U

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pointcloudcounterfactual_amd', 'csrc')
STREAM_AT = {'hipLaunchKernelGGL': 4, 'hipMemsetAsync': 3, 'hipMemcpyAsync': 4}  # the index of the stream argument
NO_STREAM = re.compile(r'^(\(\s*hipStream_t\s*\)\s*)?\(?\s*(0|nullptr|NULL)\s*\)?$')
OPEN, CLOSE = '([{', ')]}'


def _code(text):
    """``text`` without comments and string literals (their length kept, so positions stay)."""
    blank = lambda m: re.sub(r'[^\n]', ' ', m.group(0))  # noqa: E731
    text = re.sub(r'/\*.*?\*/', blank, text, flags=re.S)
    text = re.sub(r'//[^\n]*', blank, text)
    return re.sub(r'"(\\.|[^"\\\n])*"', blank, text)


def _split(text, at, close):
    """The arguments of the list that opens just before ``at``, split at depth 0, up to the closing ``close``."""
    args, depth, start, i = [], 0, at, at
    while i < len(text):
        ch = text[i]
        if depth == 0 and text.startswith(close, i):
            return args + [text[start:i].strip()]
        if ch in OPEN:
            depth += 1
        elif ch in CLOSE:
            depth -= 1
        elif ch == ',' and depth == 0:
            args.append(text[start:i].strip())
            start = i + 1
        i += 1
    raise AssertionError('an argument list that never closes')


def sites(text):
    """``(what, line, arguments)`` of every launch, async memset and async copy in ``text``."""
    text, out = _code(text), []
    for m in re.finditer(r'\b(hipLaunchKernelGGL|hipMemsetAsync|hipMemcpyAsync)\s*\(', text):
        if text[text.rfind('\n', 0, m.start()) + 1:m.start()].lstrip().startswith('#'):
            continue  # (a macro's own definition)
        out.append((m.group(1), text.count('\n', 0, m.start()) + 1, _split(text, m.end(), ')')))
    for m in re.finditer(r'<<<', text):
        out.append(('<<<', text.count('\n', 0, m.start()) + 1, _split(text, m.end(), '>>>')))
    return out


def complaint(what, args):
    """Why this site does not name a stream, or None."""
    if what == '<<<':
        if len(args) < 4:
            return 'fewer than four configuration arguments: the launch goes to the default stream'
        return 'the default stream' if NO_STREAM.match(args[3]) else None
    at = STREAM_AT[what]
    if len(args) <= at:
        return 'no stream argument: it defaults to the default stream'
    return 'the default stream' if NO_STREAM.match(args[at]) else None


def test_every_computing_symbol_is_run_by_the_stream_suite():
    from pointcloudcounterfactual_amd import _lib

    assert S.covered() == set(_lib.ABI) - U.EXEMPT, sorted(set(_lib.ABI) - U.EXEMPT - S.covered())
    assert S.CASES is U.CASES and len(S.CASES) >= 41
    assert len({s.case.name for s in S.SIZED} | {c.name for c in S.CASES}) == len(S.SIZED) + len(S.CASES)
    assert {call.symbol for s in S.SIZED for call in s.case.calls(s.case.dims)} <= S.covered()
    ring = S.ring()
    assert len(ring) == len(S.CASES) and {a.name for a, _ in ring} == {b.name for _, b in ring} and all(a is not b for a, b in ring)


def test_waits_names_existing_symbols_with_a_reason():
    from pointcloudcounterfactual_amd import _lib

    assert set(S.WAITS) <= set(_lib.ABI) - U.EXEMPT
    assert all(isinstance(reason, str) and reason.strip() for reason in S.WAITS.values())
    assert S.DELAY_MS > 0


def test_the_site_reader_sees_what_it_is_for():
    text = '''
    #define hipLaunchKernelGGL(k, ...) internal((k), __VA_ARGS__)
    // hipMemsetAsync(p, 0, n);  a comment
    hipLaunchKernelGGL((kern<1, 2>), dim3(a, b), dim3(64), 0, 0, x, f(y, z));
    hipLaunchKernelGGL(kern, grid, dim3(64), lds(n, m), st, x);
    hipMemsetAsync(p, 0xFF, bytes(n, 4));
    hipMemsetAsync(p, 0, n, nullptr);
    hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, lanes[l].st);
    kern<<<grid, 64>>>(x);
    kern<<<dim3(a, b), 64, 0, (hipStream_t)0>>>(x);
    kern<<<g, 64, 0, st>>>(x);
    '''
    got = [(what, line, complaint(what, args)) for what, line, args in sites(text)]
    assert [(w, c is None) for w, _, c in got] == [('hipLaunchKernelGGL', False), ('hipLaunchKernelGGL', True), ('hipMemsetAsync', False),
                                                   ('hipMemsetAsync', False), ('hipMemcpyAsync', True), ('<<<', False), ('<<<', False),
                                                   ('<<<', True)], got
    assert sites(text)[0][2][:2] == ['(kern<1, 2>)', 'dim3(a, b)'] and sites(text)[0][2][-1] == 'f(y, z)'


def test_no_launch_site_names_the_default_stream():
    files = sorted(f for ext in ('*.hip', '*.cpp', '*.hpp') for f in glob.glob(os.path.join(CSRC, ext)))
    assert len(files) >= 30
    found, bad = 0, []
    for path in files:
        with open(path) as f:
            for what, line, args in sites(f.read()):
                found += 1
                why = complaint(what, args)
                if why:
                    bad.append(f'{os.path.basename(path)}:{line}: {what}: {why}')
    assert found >= 100, found  # (the reader found the library's launches, not an empty tree)
    assert not bad, '\n'.join(bad)
