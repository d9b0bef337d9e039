"""_lib.launch on the device: which stream a launch reaches the library with.  A recording proxy stands
in for the object ``_lib.lib()`` returns, as in tests/test_gpu_graphed_launch_order.py, and notes the stream, the entry
point's last argument."""
import pytest
import torch

pytestmark = pytest.mark.gpu


class Recorder:
    def __init__(self, real):
        self._real, self.streams = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*a):
            self.streams.append(getattr(a[-1], "value", a[-1]) or 0)
            return fn(*a)
        return call


def test_launch_goes_on_the_current_stream_or_on_the_one_given(monkeypatch):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from nerf_simple_amd import _lib
    dev = torch.device("cuda:0")
    rec = Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    x = torch.tensor([1.5, 2.25, -0.5], dtype=torch.float32, device=dev)
    out, out2 = torch.zeros((), dtype=torch.float32, device=dev), torch.zeros((), dtype=torch.float32, device=dev)
    side, other = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    assert len({side.cuda_stream, other.cuda_stream, torch.cuda.current_stream(dev).cuda_stream}) == 3
    side.wait_stream(torch.cuda.current_stream(dev))        # x and out are filled on the current stream
    other.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        # no stream given: the current stream of dev, here side
        _lib.launch("nerf_amd_sum_f32", x, out, 3, dev=dev)
        # a stream given: that pointer arrives, whatever the current stream is
        _lib.launch("nerf_amd_sum_f32", x, out2, 3, stream=other.cuda_stream)
    assert rec.streams == [side.cuda_stream, other.cuda_stream]
    side.synchronize()
    other.synchronize()
    assert float(out) == 3.25 and float(out2) == 3.25       # exact in fp32 in any order
