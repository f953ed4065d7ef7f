"""The owner of the handle's device allocations (nexoclom_amd/csrc/nxc_devbuf.hpp) on the CPU:
tests/tools/devbuf_check.cpp instantiates it over a counting, failing fake allocator that hands out
malloc memory, so a block freed twice or never is a sanitizer report, not a GPU fault."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize('flags', [['-O1'], ['-g', '-fsanitize=address,undefined',
                                             '-fno-sanitize-recover=all']],
                         ids=['plain', 'sanitizers'])
def test_devbuf_as_a_host_program(tmp_path, flags):
    """Grow and keep, a refused allocation (flush, one retry), a refused free inside ensure and
    inside release (the buffer is empty, nothing is freed twice), release and move, and no block
    alive at any scope's end.  Built plainly and with the host sanitizers; both runs must pass."""
    exe = tmp_path / 'devbuf_check'
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', *flags,
                           os.path.join(HERE, 'tools', 'devbuf_check.cpp'), '-o', str(exe)])
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert '0 unexpected' in done.stdout and 'UNEXPECTED' not in done.stdout
    lines = done.stdout.splitlines()
    assert sum(line.endswith(' ok') for line in lines) >= 25
    assert sum('no block left' in line for line in lines) == 4
    assert not done.stderr.strip()
