"""CPU: `wave_codec.rate_pair`, the one statement of the resampler's rate-pair rule on the host, against the tap tables `resample_taps` builds
for every pair the server meets: uploads resampled to 24 kHz and the delivery rates 24 kHz PCM is resampled to."""
import pytest

from tts_indic_server_f5_amd import infer, wave_codec

PAIRS = [(o, 24000) for o in (8000, 11025, 16000, 22050, 32000, 44100, 48000)] + [(24000, r) for r in infer.OUTPUT_SAMPLE_RATES]


@pytest.mark.parametrize("orig,new", PAIRS)
def test_rate_pair_is_the_shape_of_the_tap_table(orig, new):
    of, nf, width, taps = infer.resample_taps(orig, new)
    pair = wave_codec.rate_pair(orig, new)
    assert pair[:3] == (of, nf, width)
    assert pair[3] == taps.shape[1] and taps.shape[0] == nf
    assert orig == new or pair[3] == 2 * width + of
    assert of * new == nf * orig and infer.resampled_length(of, orig, new) == nf      # reduced by the gcd


def test_equal_rates_have_no_table():
    assert wave_codec.rate_pair(24000, 24000) == (1, 1, 0, 0)
    assert infer.rate_pair is wave_codec.rate_pair
