"""`ops.ref_select` on a caller's non-default stream (tests/stream_harness.py, as tests/test_gpu_streams.py runs every other entry point): the
first call of a fresh context on a fresh side stream behind a late producer, then a second, each bit-equal to the default stream's."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ref_select_ref as S  # noqa: E402
import stream_harness as H  # noqa: E402
from tts_indic_server_f5_amd import ops  # noqa: E402


def test_ref_select_on_a_side_stream():
    clips = [S.staged(F, 7 + F) for F in (30, 19, 90)]
    lens = [len(c) for c in clips]
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist()
    wave = np.concatenate(clips)
    raw = np.clip(3.0 * wave, -1.0, 1.0)

    def run(_, t):
        tables, choices = ops.ref_select([ops.RefSelectClip(t["raw"], o, 1, n, 24000, t["wave"], o, n) for o, n in zip(off, lens)], 20, 4)
        return [*tables, choices]

    H.same_bits_on_a_side_stream("ref_select", lambda: {"raw": torch.from_numpy(raw).to("cuda:0"), "wave": torch.from_numpy(wave).to("cuda:0")}, lambda: None, run)
