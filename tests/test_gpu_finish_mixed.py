"""One `finish_requests` call with the device back-end over a micro-batch that mixes every delivery option -- plain, silence removal, G.711
with and without a loudness target, resampled PCM, FLAC at both levels and two rates, and a script -- against the same call on the host:
the bytes, the dtypes and every `backend_stats` counter.  No model: the chunk waves are noise.

Every comparison is equality: there is no tolerance anywhere."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tts_indic_server_f5_amd import infer  # noqa: E402

FADE = int(infer.cross_fade_duration * infer.target_sample_rate)   # 3600 samples
#          sample_rate, encoding, loudness, flac_level
OPTIONS = [(None, None, None, None),
           (None, None, None, None),          # the paused request, with `remove_silence`
           (8000, "mulaw", None, None),
           (8000, "mulaw", -20, None),
           (16000, "pcm16", None, None),
           (24000, "flac", None, 0),
           (24000, "flac", -16, 1),
           (16000, "flac", None, 1),
           (8000, "alaw", None, None)]         # the script
SILENCE = [i == 1 for i in range(len(OPTIONS))]


def _chunks():
    """The nine requests' chunk waves on the host: float32 noise of amplitude 0.2; request 1 with a pause of 27000 samples, request 8 a
    script of two segments."""
    rng = np.random.default_rng(0)
    noise = lambda n: rng.uniform(-0.2, 0.2, n).astype(np.float32)   # noqa: E731
    requests = [[noise(12000), noise(12000)] for _ in range(8)]
    requests[1] = [noise(36000), noise(12000)]
    requests[1][0][6000:33000] = 0.0
    requests.append([[noise(12000), noise(9000)], [noise(8000)]])
    return requests


def _finish(requests, device):
    def put(w):
        return torch.from_numpy(w).to("cuda:0") if device else w
    waves = [[put(w) for w in req] for req in requests[:8]] + [infer.SegmentedWaves([[put(w) for w in seg] for seg in requests[8]], gap_samples=2400)]
    rate, enc, loud, level = (list(col) for col in zip(*OPTIONS))
    return infer.finish_requests(waves, [""] * len(waves), infer.cross_fade_duration, SILENCE, device_backend=device, want="pcm16",
                                 sample_rate=rate, encoding=enc, loudness=loud, flac_level=level)


def test_nine_mixed_requests_in_one_device_call_equal_the_host_call():
    assert FADE == 3600
    requests = _chunks()
    host = _finish(requests, device=False)
    assert len(host[1]) == 41520 < 36000 + 12000 - FADE                      # the pause really is cut
    infer.backend_stats.clear()
    dev = _finish(requests, device=True)
    stats = dict(infer.backend_stats)
    print("backend_stats:", sorted(stats.items()))
    for i, (d, h) in enumerate(zip(dev, host)):
        assert d.dtype == h.dtype and d.shape == h.shape and d.tobytes() == h.tobytes(), (i, d.dtype, h.dtype, d.shape, h.shape)
    # nothing fell back to the host: every chunk is at least as long as the fades it takes part in
    assert stats.get("host_requests", 0) == 0
    assert stats == dict(device_calls=1, device_requests=9, loudness_calls=1, loudness_requests=2, encode_calls=4, encode_requests=5,
                         flac_calls=2, flac_requests=3, d2h_copies=9, flac_bytes=sum(len(dev[i]) for i in (5, 6, 7)))
