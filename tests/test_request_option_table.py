"""CPU: a per-request option is declared once (`infer.REQUEST_OPTIONS`, `serve.EDIT_OPTIONS`) and every route's request model has a field for
it (pydantic, like tests/test_serve.py's routes), so that a name added to the table cannot be missing from a route."""
import pytest

from tts_indic_server_f5_amd import infer, serve


def _fields(model):
    return set(getattr(model, "model_fields", None) or model.__fields__)


@pytest.mark.parametrize("name", ["KannadaSynthesizeRequest", "SynthesizeRequest", "CloneRequest"])
def test_speech_models_have_every_request_option(name):
    missing = set(infer.REQUEST_OPTIONS) - _fields(getattr(serve.request_models(), name))
    assert not missing, (name, sorted(missing))


def test_edit_model_has_every_edit_option():
    missing = set(serve.EDIT_OPTIONS + ("sample_rate", "encoding")) - _fields(serve.request_models().EditRequest)
    assert not missing, sorted(missing)
