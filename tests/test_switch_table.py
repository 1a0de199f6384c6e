"""The library's switches and shared host helpers each live in ONE place (text only, no GPU).

* Every ``NJODE_*`` variable the C++ reads is parsed in ``njode_amd/csrc/njode_env.h``; the variable column
  of the table in DESIGN.md section 4g names exactly those.
* No other file under ``njode_amd/csrc`` reads the environment.
* ``fail()``, ``HIP_TRY`` and ``ProfScope`` are each defined in exactly one file.
"""
import glob
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'njode_amd', 'csrc')


def sources():
    out = {}
    for path in sorted(glob.glob(os.path.join(CSRC, '*.h')) + glob.glob(os.path.join(CSRC, '*.hip'))):
        with open(path) as f:
            out[os.path.basename(path)] = f.read()
    return out


def table_variables():
    with open(os.path.join(REPO, 'DESIGN.md')) as f:
        text = f.read()
    section = text.split('### 4g.', 1)[1].split('\n## ', 1)[0]
    rows = [l for l in section.splitlines() if l.startswith('| `NJODE_')]
    assert rows, 'DESIGN.md section 4g has no switch table'
    names = []
    for row in rows:
        names += re.findall(r'`(NJODE_[A-Z0-9_]+)`', row.split('|')[1])
    return names


def test_env_header_and_design_table_name_the_same_switches():
    parsed = re.findall(r'"(NJODE_[A-Z0-9_]+)"', sources()['njode_env.h'])
    assert len(parsed) == len(set(parsed)), 'a switch is parsed twice: {}'.format(
        sorted(n for n in set(parsed) if parsed.count(n) > 1))
    table = table_variables()
    assert len(table) == len(set(table)), 'a switch has two rows'
    assert set(parsed) == set(table), (sorted(set(parsed) - set(table)), sorted(set(table) - set(parsed)))


def test_only_the_env_header_reads_the_environment():
    readers = [name for name, text in sources().items() if 'getenv(' in text]
    assert readers == ['njode_env.h'], readers


def test_shared_host_helpers_are_defined_once():
    src = sources()
    for what, pattern in (('fail(', r'^\s*(?:static\s+|inline\s+)*int\s+fail\s*\('),
                          ('HIP_TRY', r'^\s*#\s*define\s+HIP_TRY\b'),
                          ('struct ProfScope', r'^\s*struct\s+ProfScope\b')):
        where = [name for name, text in src.items() if re.search(pattern, text, re.M)]
        assert where == ['njode_hostlib.h'], (what, where)
