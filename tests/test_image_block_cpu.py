"""The image-shaped LDS block of nxc_set_image and nxc_camera_set, without a GPU."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_image_block_builder_as_a_host_program(tmp_path):
    """Appending [g-value tables | first edges | second edges] to a byte block and placing it at
    an offset of the LDS are host-only code (nxc_image_block.hpp) that the model image uses twice
    and the camera once; tests/tools/image_block_check.cpp builds blocks of 0, 1 and NXC_MAX_LINES
    tables with 1 x 1 and 512 x 800 edges, places them at several bases and checks offsets, sizes,
    bytes and that every placed table lies inside the block.  Built plainly here; the same file is
    what is built with -fsanitize=address,undefined."""
    exe = tmp_path / 'image_block_check'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror',
                           os.path.join(HERE, 'tools', 'image_block_check.cpp'), '-o', str(exe)])
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout
    assert done.stdout.strip() == '12 blocks, 48 placements, 0 unexpected'
