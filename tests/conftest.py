import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pytest_configure(config):
    config.addinivalue_line(
        "markers", "gpu: needs a real MI355X GPU (run via gpurun / driver)"
    )


@pytest.fixture(autouse=True)
def _cpu_tests_start_cpu_processes(request, monkeypatch):
    """A test without the gpu marker is a CPU test wherever it runs: the
    processes it starts (launchers, bench.py, the examples) must not pick up
    a GPU that happens to be there — two CPU/gloo ranks on a one-GPU machine
    would ask for cuda:1.  Only child processes are affected: this process
    has read the device list already (pytest_collection_modifyitems)."""
    if "gpu" not in request.keywords:
        monkeypatch.setenv("HIP_VISIBLE_DEVICES", "-1")
        monkeypatch.setenv("CUDA_VISIBLE_DEVICES", "-1")
    yield


def pytest_collection_modifyitems(config, items):
    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="no GPU in this container")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)
