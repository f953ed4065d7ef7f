"""Which instantiation of k_const_fused a launch gets, and the LDS it asks for, without a GPU."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_fused_variant_choice_as_a_host_program(tmp_path):
    """The choice of the kernel variant from a launch's flags, the variants' codes (from which
    nxc_api.hip generates its table of kernels), which of them exist and the LDS size of a
    persistent workgroup are host-only code (nxc_fused_variant.hpp); tests/tools/
    fused_variant_check.cpp compares them with tables written out there, over every combination
    of flags.  Built plainly here; the same file is what is built with
    -fsanitize=address,undefined."""
    exe = tmp_path / 'fused_variant_check'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror',
                           os.path.join(HERE, 'tools', 'fused_variant_check.cpp'), '-o', str(exe)])
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout
    assert done.stdout.strip() == ('768 flag combinations, 31 valid variants of 144 codes, '
                                   '31 reachable, 0 unexpected')
