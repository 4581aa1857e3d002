"""The formant shift (`wave_codec.psola_shape_pcm16`) restated sample by sample in plain Python integers, on top of `formant_ref`'s track
and marks: one loop over the synthesis marks and their output offsets, nothing shared with `wave_codec` or the kernels."""
import formant_ref as ref


def synthesis(marks, n, semitones):
    """`formant_ref.synthesis_marks`; without a pitch (p = q = 1) every step is the period of the mark it took."""
    if semitones:
        return ref.synthesis_marks(marks, n, semitones)
    out, u = [], marks[0][0] if marks else n
    while u < n:
        out.append((u, min(range(len(marks)), key=lambda k: (abs(marks[k][0] - u), k))))
        u += marks[out[-1][1]][1]
    return out


def shape(x, marks, semitones, formant):
    """The n output samples of the list of ints x under its analysis marks [(a, T, voiced)]."""
    n, M = len(x), ref.window()
    xt = lambda j: x[j] if 0 <= j < n else 0   # noqa: E731
    P, Q = ref.ratio(formant).as_integer_ratio() if formant else (1, 1)
    num, den = [0] * n, [0] * n
    for u, i in synthesis(marks, n, semitones):
        a, T, voiced = marks[i]
        Pg = P if voiced else Q                                             # an unvoiced grain is not shifted: v = x Q
        for k in range(-(T * Q // Pg), T * Q // Pg + 1):
            if 0 <= u + k < n:
                c, r = divmod(k * Pg, Q)
                num[u + k] += M[(abs(k) * Pg * ref.TABLE) // (Q * T)] * (xt(a + c) * (Q - r) + xt(a + c + 1) * r)
                den[u + k] += M[(abs(k) * Pg * ref.TABLE) // (Q * T)] * Q
    return [min(max(x[j] if den[j] == 0 else (2 * num[j] + den[j]) // (2 * den[j]), -32768), 32767) for j in range(n)]
