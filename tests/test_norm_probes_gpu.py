"""Per-hop probes of the feature normaliser on the MI355X (libnmx.so): the five scan kernels at their segment, piece and
16-bit count edges, the column walk (naturally and with NMX_NORM_SCAN=0), the sorted-list family, the Yeo-Johnson fit and
the device-memory call shape, every output against the float64 hop-by-hop oracle; on the mean / zscore columns that allow
it within one fp32 ulp, which is what sees the hardware-seeded float64 reciprocal and reciprocal square root that the
emulator compiles out.  Cases and policy: tests/norm_probe_cases.py; no miss is accepted; figures: profiles/norm_probes.md."""

import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import norm_probe_cases as cases  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]


@pytest.fixture(scope="module", autouse=True)
def gpu_lib():
    from py_neuromodulation_amd import _lib

    lib = _lib.get_library()
    assert lib.device_count() >= 1, "no HIP device visible"
    assert "libnmx.so" in str(lib.path)
    return lib


def torch_tensor_on_a_side_stream(dn, buf):
    import torch

    t = torch.from_numpy(buf).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    dn.process_device(t.data_ptr(), buf.shape[1], buf.shape[0], side.cuda_stream)
    side.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize("name", list(cases.SCAN_CASES))
def test_scan_geometry(monkeypatch, name):
    print(name, cases.mz_case(None, name, True, monkeypatch))


@pytest.mark.parametrize("name", list(cases.WALK_CASES))
def test_walk(monkeypatch, name):
    print(name, cases.mz_case(None, name, True, monkeypatch))


@pytest.mark.parametrize("name", cases.SCAN_OFF_CASES)
def test_walk_on_the_scan_inputs(monkeypatch, name):
    print(name, cases.mz_case(None, name, False, monkeypatch))


@pytest.mark.parametrize("first_scan", [True, False])
def test_state_crosses_between_scan_and_walk(monkeypatch, first_scan):
    cases.state_crossing_case(None, monkeypatch, first_scan)


@pytest.mark.parametrize("kind", ["scan", "walk", "power"])
def test_device_call_shape_with_guard_columns(monkeypatch, kind):
    cases.device_shape_case(None, monkeypatch, kind, torch_tensor_on_a_side_stream)


@pytest.mark.parametrize("method", cases.ORDER_METHODS)
@pytest.mark.parametrize("name", list(cases.ORDER_CASES))
def test_order_family(name, method):
    print(name, method, cases.order_case(None, name, method))


@pytest.mark.parametrize("method,n_cols", cases.ORDER_WIDE)
def test_order_family_wide(method, n_cols):
    print(method, n_cols, cases.order_case(None, "o50", method, clips=(3,), n_cols=n_cols))


@pytest.mark.parametrize("name", list(cases.POWER_CASES))
def test_power(name):
    print(name, cases.power_case(None, name))
