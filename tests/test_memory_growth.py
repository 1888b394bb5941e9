"""The growth helper of csrc/pt_memory.hpp where there is no device: pt_memory_check (csrc/Makefile builds it next to pt_demo) then
checks the all-fail half of the contract -- every call fails, every buffer stays empty. With a device the program walks the whole
contract instead; that run is tests/test_memory_growth_gpu.py's."""
import os
import subprocess

import pytest

import __graft_entry__ as ge

CHECK = os.path.join(ge.PKG_DIR, "pt_memory_check")


def run_check():
    """(exit status, the lines of the report)"""
    p = subprocess.run([CHECK], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(p.stdout)
    return p.returncode, p.stdout.splitlines()


def test_growth_without_a_device_fails_whole_and_leaves_every_buffer_empty():
    status, lines = run_check()
    if lines and lines[0] == "mode: device":
        pytest.skip("pt_memory_check found a device: the no-device half is checked where there is none")
    assert lines[0] == "mode: no device"
    steps = lines[1:]
    assert len(steps) == 5 and all(s.startswith("ok: ") for s in steps), steps
    assert status == 0
