"""GPU: a non-finite request costs that request only -- not the other requests of its batch, not the requests that use the handle afterwards.

One handle serves every request of a process, `ContinuousBatcher` packs unrelated requests into one sampler call, `decode_ragged` packs
unrelated chunks into one vocoder call, and nothing on the path rejects a non-finite mel.  The "item equals the same item alone" tests of
the ragged paths all use finite values, and a leak that is masked by MULTIPLICATION (a probability of exactly 0 times a neighbour's value
row, a zero weight times a halo row, a statistic summed one row too far) changes nothing there, or a last bit inside a tolerance.  With a
NaN neighbour it destroys the row.  So here the neighbours are poison: NaN, and 1e30 (finite, but it overflows every fp16 conversion and
every sum of squares), each as its own case.  Every comparison is `torch.equal` unless it names the oracle.

Same call: units A | B | C (items, for the vocoders) run twice with identical shapes and arguments, A and C finite in the first run and
poisoned in the second; B's output must be bit-identical.  The shapes are the same in both runs, so the same kernels run and the
shape-invariant attention mode is not needed.
Next call: a small probe, a larger poisoned call that reallocates the grow-only workspace and writes every buffer beyond the probe's
layout, the probe again, a refused call, the probe again: all probe results bit-equal to each other and to a FRESH handle's (whose
workspace is zeroed, so agreement with it cannot be a shared mistake), one probe per handle anchored against its fp64 oracle.

NaN is only ever data on these paths (read before the first run: csrc/attn3.h, f5hip.hip, cfm_sample.h, elementwise.h, ln_row.h,
vocos.h, bigvgan.h): every trip count, index and address comes from the integer metadata of the layout; float values reach comparisons
only in selects (the key mask, clamps) and in attn3's redo vote, which sends inf / NaN row sums to ONE running-maximum pass."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import bigvgan_oracle as B  # noqa: E402
from oracle import dit_oracle as O  # noqa: E402
from oracle import vocos_oracle as V  # noqa: E402
from test_gpu_request_knobs import _backbone, _rms  # noqa: E402
from tts_indic_server_f5_amd import _lib, synth  # noqa: E402

FILLS = [float("nan"), 1e30]
FILL_IDS = ["nan", "1e30"]
KINDS = ["dit", "unett", "mmdit"]
VOCAB = {chr(65 + i): i for i in range(40)}   # the tiny backbones' 40 token ids as characters (sample_units takes token lists)
# B's rows: 41; exactly one and two 128-row pitches (UNetT: the time token takes a row), between neighbours that end on the pitch too, so no
# padding row lies between B and a poisoned row (the position-embedding convolutions' halos, the text ConvNeXt's k = 7 window, the GRN sums);
# 129, which pads to 256 rows
B_DURS = {"dit": [41, 128, 256, 129], "unett": [41, 127, 255, 129], "mmdit": [41, 128, 256, 129]}


def _same(a, b, tag):
    assert a.shape == b.shape, f"{tag}: {tuple(a.shape)} vs {tuple(b.shape)}"
    if not torch.equal(a, b):
        bad = (a != b) | torch.isnan(a) | torch.isnan(b)
        rows = bad.reshape(bad.shape[0], -1).any(dim=1).nonzero().flatten().tolist()
        raise AssertionError(f"{tag}: {len(rows)} of {bad.shape[0]} rows differ (rows {rows[0]}..{rows[-1]}), {int(torch.isnan(a).sum())} NaN, "
                             f"max diff {(a - b).abs().nan_to_num(float('inf')).max().item():.3e}")


def _model(kind, planes, **kw):
    from tts_indic_server_f5_amd.model import F5HipModel
    arch, sd, _, _ = _backbone(kind)
    return F5HipModel(arch, sd, vocab_char_map=VOCAB, gemm_planes=planes, **kw)


# ---------------------------------------------------------------------------------------------------------------- sampler units
def _unit(g, prompt, n_text, dur):
    """(prompt mel [1, prompt, 100], token ids [1, n_text], planned frames = final rows, noise [dur, 100])"""
    assert dur >= max(prompt, n_text) + 1
    return (torch.randn(1, prompt, 100, generator=g), torch.randint(0, 40, (1, n_text), generator=g), dur, torch.randn(dur, 100, generator=g))


def _poisoned(u, fill):
    cond, text, dur, y0 = u
    return (torch.full_like(cond, fill), text, dur, torch.full_like(y0, fill))


def _abc(kind, b_dur):
    """A | B | C: A and C end on the 128-row pitch; MMDiT's B carries a text of exactly 128 tokens where its rows allow it"""
    g = torch.Generator().manual_seed(900 + b_dur)
    pitch = 127 if kind == "unett" else 128
    n_text = 128 if kind == "mmdit" and b_dur >= 129 else 10
    return [_unit(g, 24, 12, pitch), _unit(g, 12, n_text, b_dur), _unit(g, 18, 8, pitch)]


def _sample(model, units, **kw):
    pad = torch.nn.utils.rnn.pad_sequence
    conds = pad([u[0][0] for u in units], batch_first=True)
    texts = pad([u[1][0] for u in units], batch_first=True, padding_value=-1)
    kw.setdefault("sway_sampling_coef", -1.0)
    out, _ = model.sample(conds, texts, torch.tensor([u[2] for u in units]), lens=torch.tensor([u[0].shape[1] for u in units]),
                          y0=[u[3] for u in units], **kw)
    return [out[i, :u[2]] for i, u in enumerate(units)]


def _one_grid(model, units):
    toks = [[chr(65 + int(i)) for i in u[1][0]] for u in units]
    return model.sample_units([u[0] for u in units], [(t, u[2]) for t, u in zip(toks, units)], steps=3, cfg_strength=2.0, sway_sampling_coef=-1.0,
                              y0=[u[3] for u in units])


def _edit_mask(model, units):
    em = torch.ones(len(units), max(max(u[0].shape[1], u[1].shape[1]) for u in units), dtype=torch.bool)
    em[:, 3:8] = False   # frames 3..7 of every prompt are regenerated
    return _sample(model, units, steps=3, cfg_strength=2.0, edit_mask=em)


def _spans(model, units):
    planned = [model.plan_unit(u[0], u[1][0], u[2], steps=4, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=u[3]) for u in units]
    assert model.advance(planned, 2) == []
    assert model.advance(planned, 2) == planned
    return [p.mel for p in planned]


# entry point -> fn(model, [A, B, C]) -> their outputs [dur, 100]
ENTRIES = {
    "one_grid": _one_grid,                                                                        # sample_units -> f5hip_cfm_sample_masked
    "edit_mask": _edit_mask,
    "cfg_b0": lambda m, u: _sample(m, u, steps=3, cfg_strength=[2.0, 0.0, 3.5]),   # B without an unconditional sequence
    "cfg_a0": lambda m, u: _sample(m, u, steps=3, cfg_strength=[0.0, 2.0, 3.5]),   # a poisoned unit without one
    # per-row time tables and the shrinking prefix of finished units: the poisoned units finish first / last
    "steps_poison_first": lambda m, u: _sample(m, u, steps=[2, 4, 2], cfg_strength=2.0, sway_sampling_coef=[-1.0, None, 0.5]),
    "steps_poison_last": lambda m, u: _sample(m, u, steps=[4, 2, 4], cfg_strength=2.0, sway_sampling_coef=[-1.0, None, 0.5]),
    "methods": lambda m, u: _sample(m, u, steps=2, cfg_strength=2.0, ode_method=["rk4", "midpoint", "euler"]),
    "methods_b_rk4": lambda m, u: _sample(m, u, steps=2, cfg_strength=[2.0, 2.0, 0.0], ode_method=["euler", "rk4", "midpoint"]),
    "spans": _spans,                                                                              # plan_unit / advance, two spans
}


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("planes", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_sampler_unit_between_poisoned_units(kind, planes, entry, fill):
    """One call holds A | B | C, run twice on one handle: all finite, then A's and C's `cond` and `y0` poisoned.  B's output is bit-identical,
    for every length of B (B_DURS).  Under NaN the generated frames of A and C come out NaN: the poison went in.  The finite run of the next
    length follows a poisoned call on the same handle, so a finite B there also shows that nothing stayed behind.
    `padded_batch=True` is left out: it reproduces the reference's own leak through unmasked padding
    (test_padded_batch_sampler_vs_reference_fixture pins it)."""
    model = _model(kind, planes)
    nan_frames = []
    for b_dur in B_DURS[kind]:
        a, b, c = _abc(kind, b_dur)
        clean = ENTRIES[entry](model, [a, b, c])
        dirty = ENTRIES[entry](model, [_poisoned(a, fill), b, _poisoned(c, fill)])
        tag = f"{kind} planes {planes} {entry} B = {b_dur} rows, fill {fill}"
        assert torch.isfinite(clean[1]).all(), tag
        if math.isnan(fill):
            for u, out in ((a, dirty[0]), (c, dirty[2])):
                assert torch.isnan(out[u[0].shape[1]:]).any(), f"{tag}: a poisoned unit's generated frames hold no NaN"
            nan_frames.append(int(torch.isnan(torch.cat([dirty[0], dirty[2]])).any(dim=1).sum()))
        _same(dirty[1], clean[1], f"{tag}: B between poisoned units vs between finite ones")
    print(f"[isolation] sampler {kind} planes {planes} {entry} fill {fill}: B of {B_DURS[kind]} rows bit-equal between poisoned and finite A / C"
          + (f"; NaN frames of A and C: {nan_frames}" if nan_frames else ""))


# ---------------------------------------------------------------------------------------------------------------- sampler, next call
def _probe_units():
    g = torch.Generator().manual_seed(940)
    return [_unit(g, 24, 12, 60), _unit(g, 12, 10, 41), _unit(g, 18, 8, 45)]


def _forward_probe(model, kind):
    """transformer_forward stopped behind block 1 + the text tap of that layout, then the whole forward.  MMDiT's tap is the text slab as
    laid out; only its token rows are compared: text_gather_kernel skips the slab's padding rows, which keep what an earlier layout left
    there (text-derived, so never poison, and masked as keys)."""
    g = torch.Generator().manual_seed(941)
    x, cond, text = torch.randn(2, 41, 100, generator=g), torch.randn(2, 41, 100, generator=g), torch.randint(0, 40, (2, 12), generator=g)
    h = model.transformer_forward(x, cond, text, 0.37, False, False, n_blocks=1)
    if kind == "mmdit":   # the text stream's embedding as laid out: 12 tokens at the head of a 128-row slab per sequence
        rows = model.read_tap("text_rows", 256, model.arch.dim)
        tap = torch.cat([rows[0:12], rows[128:140]])
    else:
        tap = model.read_tap("text_embed", 2 * 41, model.arch.text_dim)
    return [h.reshape(82, -1), tap, model.transformer_forward(x, cond, text, 0.37, False, False).reshape(82, -1)]


def _run_probes(model, kind):
    out = {name: [t.clone() for t in fn(model, _probe_units())] for name, fn in ENTRIES.items()}
    out["forward_taps"] = [t.clone() for t in _forward_probe(model, kind)]
    return out


_FRESH = {}


def _fresh_probes(kind, planes):
    """Every probe on a handle of its own that has run nothing else (workspace zeroed at allocation); computed once, never modified"""
    key = (kind, planes)
    if key not in _FRESH:
        res = {}
        for name, fn in ENTRIES.items():
            res[name] = [t.clone() for t in fn(_model(kind, planes), _probe_units())]
        res["forward_taps"] = [t.clone() for t in _forward_probe(_model(kind, planes), kind)]
        _FRESH[key] = res
    return _FRESH[key]


def _assert_probes(got, want, tag):
    assert got.keys() == want.keys()
    for name in want:
        for i, (a, b) in enumerate(zip(got[name], want[name])):
            _same(a, b, f"{tag}: probe {name} output {i} vs a fresh handle")


def _span_start(model):
    planned = [model.plan_unit(u[0], u[1][0], u[2], steps=4, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=u[3]) for u in _probe_units()]
    assert model.advance(planned, 2) == []
    return planned


def _span_finish(model, planned, want, tag):
    assert model.advance(planned, 2) == planned
    for i, (p, w) in enumerate(zip(planned, want)):
        _same(p.mel, w, f"{tag}: span pair around it, unit {i} vs a fresh handle")


def _history(model, fill):
    """More units, longer ones and longer texts than any probe, all poisoned, through the per-unit plan (every ODE buffer, the grid tables)
    and through a whole forward: the workspace is reallocated and every buffer beyond the probes' layouts written."""
    g = torch.Generator().manual_seed(942)
    units = [_poisoned(_unit(g, 30, 140, d), fill) for d in (300, 290, 200, 280, 150)]
    outs = _sample(model, units, steps=[2, 2, 3, 2, 2], cfg_strength=2.0, ode_method=["rk4", "midpoint", "euler", "rk4", "euler"])
    x = torch.full((5, 300, 100), fill)
    full = model.transformer_forward(x, x, torch.randint(0, 40, (5, 140), generator=g), 0.5, False, False)
    if math.isnan(fill):
        assert all(torch.isnan(o[30:]).any() for o in outs) and torch.isnan(full).any(), "the history calls hold no NaN: the poison never went in"


def _refused(model, durs):
    """A call with a token outside the vocabulary: refused inside setup_sequences, behind ensure_workspace"""
    g = torch.Generator().manual_seed(943)
    units = [_unit(g, 24, 12, d) for d in durs]
    units[-1][1][0, 5] = 40   # the vocabulary is 0..39
    with pytest.raises(_lib.F5HipError, match="outside the vocabulary"):
        _sample(model, units, steps=3, cfg_strength=2.0)


def _dit_rows():
    v = C.c_int64(0)
    _lib.check(_lib.lib().f5hip_get_counter(b"dit_rows", C.byref(v)), "get_counter")
    return v.value


_ORACLE = {}


def _oracle_unit_b(kind):
    """The fp64-pinned CPU oracle's sampler on unit B of the probes, as the one-grid probe samples it"""
    if kind not in _ORACLE:
        _, sd, fwd, cfg = _backbone(kind)
        cond, text, f, y0 = _probe_units()[1]
        ref, _ = O.cfm_sample(sd, cfg, cond, text, f, steps=3, cfg_strength=2.0, sway_sampling_coef=-1.0, y0=y0[None], forward_fn=fwd,
                              keep_trajectory=False)
        _ORACLE[kind] = ref[0]
    return _ORACLE[kind]


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("planes", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_sampler_next_call_after_poisoned_and_refused_calls(kind, planes, fill):
    """On ONE handle: probes | larger poisoned history | probes | refused call of the probes' size | probes | refused call larger than
    everything before (ensure_workspace grows the arena, then setup_sequences refuses) | probes.  The probes are every entry point of the
    same-call test on three small finite units, transformer_forward(n_blocks=1) with its text tap and the whole forward, and a span pair
    with the history call (and each refused call) BETWEEN its two advance calls.  All bit-equal to a fresh handle's; the one-grid probe's
    unit B within 1e-3 rms of the oracle's sampler (north_star's mel bound, as in tests/test_gpu_request_knobs.py).  The refused calls
    run no backbone row ("dit_rows")."""
    fresh = _fresh_probes(kind, planes)
    model = _model(kind, planes)
    tag = f"{kind} planes {planes} fill {fill}"
    _assert_probes(_run_probes(model, kind), fresh, tag + ", first use")
    pair = _span_start(model)
    _history(model, fill)
    _span_finish(model, pair, fresh["spans"], tag + ", poisoned history")
    after = _run_probes(model, kind)
    _assert_probes(after, fresh, tag + ", after the poisoned history")
    for what, durs in (("refused call", (60, 41, 45)), ("refused call that grows the workspace", (400,) * 6)):
        pair = _span_start(model)
        rows = _dit_rows()
        _refused(model, durs)
        assert _dit_rows() == rows, f"{tag}: the {what} ran backbone rows"
        _span_finish(model, pair, fresh["spans"], f"{tag}, {what}")
        _assert_probes(_run_probes(model, kind), fresh, f"{tag}, after the {what}")
    b = _probe_units()[1]
    p = b[0].shape[1]
    rms = _rms(after["one_grid"][1][p:], _oracle_unit_b(kind)[p:])
    print(f"[isolation] sampler next call {tag}: {len(fresh)} probes x 4 rounds and 3 span pairs bit-equal to a fresh handle; "
          f"one-grid probe unit B after the history, rms vs oracle {rms:.3e} (bound 1e-3)")
    assert rms < 1e-3


# ---------------------------------------------------------------------------------------------------------------- vocoders
BV_C0, BV_UP = 256, 256                      # the reduced generator of tests/test_gpu_bigvgan_ragged.py
FRAMES = [1, 5, 127, 128, 129, 37]           # its items: on, just before and just after the 128-row pitch; one frame; two short ones
# Vocos refuses an item of one frame (its wave has hop (T - 1) = 0 samples; test_vocos_refuses_the_one_frame_item): 2 frames stand in
VOCOS_FRAMES = [2, 5, 127, 128, 129, 37]
VOCODERS = [("vocos", 2), ("vocos", 1), ("bigvgan", 2), ("bigvgan", 3), ("bigvgan", 1)]   # every gemm_planes of each
VOC_IDS = [f"{n}-planes{p}" for n, p in VOCODERS]


@pytest.fixture(scope="module")
def voc_sd():
    return {"vocos": synth.vocos_state_dict(), "bigvgan": synth.bigvgan_state_dict(upsample_initial_channel=BV_C0)}


def _vocoder(voc_sd, name, planes):
    from tts_indic_server_f5_amd.vocoder import F5HipBigVGAN, F5HipVocos
    if name == "vocos":
        return F5HipVocos(voc_sd[name], gemm_planes=planes)
    return F5HipBigVGAN(voc_sd[name], upsample_initial_channel=BV_C0, gemm_planes=planes)


def _own_call(voc, name, mel):
    return (voc.decode(mel[None]) if name == "vocos" else voc(mel[None])).reshape(-1).clone()


def _mels(frames, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(100, t, generator=g) * 1.5 - 1.0 for t in frames]


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("name,planes", VOCODERS, ids=VOC_IDS)
def test_vocoder_items_between_poisoned_items(voc_sd, name, planes, fill):
    """decode_ragged over the six items with every other one poisoned -- the odd ones, then the even ones, which gives the 128-frame item a
    poisoned neighbour on each side in turn: each finite item is bit-equal to the same item of the all-finite call AND to its own call.
    (Channels: the depthwise k = 7 window, the iSTFT overlap-add at item seams; the anti-aliased snake's 12 taps, the dilated halos up to 25
    rows, the up-samplers' three taps and conv_post's seven.)  A poisoned item's own wave is NaN from Vocos; BigVGAN's conv_post ends in
    clamp(-1, 1), which maps NaN to a bound, so there the poisoned item merely has to differ from its finite wave."""
    voc = _vocoder(voc_sd, name, planes)
    frames = VOCOS_FRAMES if name == "vocos" else FRAMES
    mels = _mels(frames, 511)
    clean = [w.clone() for w in voc.decode_ragged(mels)]
    for parity in (1, 0):
        dirty = voc.decode_ragged([torch.full_like(m, fill) if i % 2 == parity else m for i, m in enumerate(mels)])
        for i, (t, m) in enumerate(zip(frames, mels)):
            tag = f"{name} planes {planes} fill {fill}, items {parity} mod 2 poisoned, item {i} (T = {t})"
            if i % 2 == parity:
                if name == "vocos" and math.isnan(fill):
                    assert torch.isnan(dirty[i]).any(), f"{tag}: the poisoned item's wave holds no NaN"
                else:
                    assert not torch.equal(dirty[i], clean[i]), f"{tag}: the poisoned item's wave did not change"
                continue
            assert torch.isfinite(clean[i]).all(), tag
            _same(dirty[i], clean[i], f"{tag} vs the all-finite call")
            _same(dirty[i], _own_call(voc, name, m), f"{tag} vs its own call")
    print(f"[isolation] {name} planes {planes} fill {fill}: items of {frames} frames, odd then even ones poisoned: every finite item bit-equal "
          f"to the all-finite call and to its own call")


def test_vocos_refuses_the_one_frame_item(voc_sd):
    voc = _vocoder(voc_sd, "vocos", 2)
    with pytest.raises((_lib.F5HipError, RuntimeError), match="frames"):
        voc.decode_ragged(_mels([5, 1], 512))


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("name,planes", VOCODERS, ids=VOC_IDS)
def test_vocoder_next_call_after_poisoned_and_refused_calls(voc_sd, name, planes, fill):
    """On ONE vocoder: probe (a ragged call of two short items and a uniform batch of 2) | a poisoned ragged call with more and longer items,
    which reallocates the workspace and writes every row beyond the probe's | probe | refused calls | probe: all bit-equal to a fresh
    object's.  In the parity mode (gemm_planes 2) the probe's items are also held to the float64 oracle at the existing bounds: 1e-4 max
    on waveform samples (tests/test_gpu_vocos.py, tests/test_gpu_bigvgan_ragged.py)."""
    short = _mels([5, 37], 513)
    uni = torch.stack(_mels([13, 13], 514))

    def probe(v):
        batch = v.decode(uni) if name == "vocos" else v(uni)
        return [w.clone() for w in v.decode_ragged(short)] + [batch.reshape(2, -1).clone()]

    fresh = probe(_vocoder(voc_sd, name, planes))
    voc = _vocoder(voc_sd, name, planes)

    def check(when):
        for i, (a, b) in enumerate(zip(probe(voc), fresh)):
            _same(a, b, f"{name} planes {planes} fill {fill}, {when}: probe output {i} vs a fresh object")

    check("first use")
    history = voc.decode_ragged([torch.full((100, t), fill) for t in (129, 128, 127, 200, 60, 300)])
    if name == "vocos" and math.isnan(fill):
        assert all(torch.isnan(w).any() for w in history)
    check("after the poisoned history")
    with pytest.raises((_lib.F5HipError, RuntimeError)):
        voc.decode_ragged([short[0], torch.zeros(100, 0)])
    f = torch.tensor([5, 0], dtype=torch.int32)   # the C entry point itself: an item without frames
    x, w = torch.zeros(2, 100, 5, device="cuda"), torch.zeros(BV_UP * 5, device="cuda")
    entry = _lib.lib().f5hip_vocos_decode_ragged if name == "vocos" else _lib.lib().f5hip_bigvgan_forward_ragged
    assert entry(voc._h, 2, C.c_void_p(f.data_ptr()), C.c_void_p(x.data_ptr()), C.c_void_p(w.data_ptr()), _lib.current_stream_ptr()) != 0
    check("after the refused calls")
    if planes != 2:
        return
    sd = voc_sd[name]
    for m, got in zip(short, probe(voc)):
        if name == "vocos":
            ref = V.vocos_decode(sd, m[None]).reshape(-1)
        else:
            ref = B.bigvgan_forward({k: v.double() for k, v in sd.items()}, B.BigVGANConfig(upsample_initial_channel=BV_C0), m[None].double()).reshape(-1)
        mx = (got.cpu().double() - ref.double()).abs().max().item()
        print(f"[isolation] {name} next call fill {fill}: probe item T = {m.shape[1]} after the history and the refusals, max err vs the oracle "
              f"{mx:.3e} (bound 1e-4)")
        assert mx < 1e-4


# ---------------------------------------------------------------------------------------------------------------- mel tables
def test_mel_front_end_tables_survive_a_change_of_geometry():
    """The mel front-ends rebuild process-wide tables when (n_mels, sample_rate) changes: parameter sets X, Y, X, Y through both front-ends
    (and the ragged launch, which shares the tables) -- the third result equals the first and the fourth the second, bit for bit."""
    from tts_indic_server_f5_amd.mel import mel_spectrogram, mel_spectrogram_bigvgan, mel_spectrogram_ragged
    wave = synth.ref_audio(24000, amp=0.15).cuda()
    X, Y = dict(n_mel_channels=100, target_sample_rate=24000), dict(n_mel_channels=80, target_sample_rate=16000)
    for variant, fe in (("vocos", mel_spectrogram), ("bigvgan", mel_spectrogram_bigvgan)):
        x1, y1, x2, y2 = fe(wave, **X), fe(wave, **Y), fe(wave, **X), fe(wave, **Y)
        assert x1.shape[1] == 100 and y1.shape[1] == 80 and torch.isfinite(x1).all() and torch.isfinite(y1).all()
        assert not torch.equal(x1[:, :80], y1), variant
        _same(x2, x1, f"{variant} front-end: X after Y")
        _same(y2, y1, f"{variant} front-end: Y after X")
        rag, _ = mel_spectrogram_ragged([wave[0]], variant, **X)
        _same(rag, x1[0].T.contiguous(), f"{variant} front-end: the ragged launch at X after Y")
