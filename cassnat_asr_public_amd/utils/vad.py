"""Host side of the energy VAD (``bin/make_segments``): Kaldi's option file of `compute-vad-decision` and the segmentation of one
byte per frame.  The per-sample work - frame energies and the decision - runs on the device (``hip.frame_energy`` / ``hip.vad_decide``;
include/cassnat_hip_vad.h); what is left here is list arithmetic on runs of frames.  Not in the reference.

Segmentation, all in frames (seconds become frames by ``frames_of_seconds``: round(sec / shift_sec)):
  1. the maximal runs [a, b) of dec == 1;
  2. neighbours whose gap is shorter than ``min_silence`` are merged;
  3. runs shorter than ``min_speech`` are dropped;
  4. both ends move out by ``pad``, clipped to [0, T); where two padded neighbours would overlap both ends move to
     floor((b_i + a_{i+1}) / 2) of the unpadded ends;
  5. while a run is longer than ``max_segment`` frames M it is cut at the FIRST minimum of e over [a + M // 2, a + M), and the rest
     goes on."""

VAD_OPTIONS = {"vad-energy-threshold": ("thr0", float), "vad-energy-mean-scale": ("mean_scale", float), "vad-frames-context": ("context", int),
               "vad-proportion-threshold": ("proportion", float)}
VAD_DEFAULTS = {"thr0": 5.0, "mean_scale": 0.5, "context": 0, "proportion": 0.6}  # Kaldi's
MAX_CONTEXT = 64


def parse_vad_conf(path):
    """A Kaldi option file (`--name=value` lines, blank lines, `#` comments) of compute-vad-decision -> the four options over Kaldi's
    defaults; any other option raises a ValueError that names it."""
    opts = dict(VAD_DEFAULTS)
    if not path:
        return opts
    with open(path) as f:
        for raw in f:
            line = raw.split("#", 1)[0].strip()
            if not line:
                continue
            if not line.startswith("--") or "=" not in line:
                raise ValueError("vad conf %s: not a --name=value line: %r" % (path, raw.rstrip("\n")))
            name, _, text = line[2:].partition("=")
            name, text = name.strip(), text.strip()
            if name not in VAD_OPTIONS:
                raise ValueError("vad conf %s: unknown option --%s (known: %s)" % (path, name, ", ".join("--" + n for n in sorted(VAD_OPTIONS))))
            key, kind = VAD_OPTIONS[name]
            try:
                opts[key] = kind(text)
            except ValueError:
                raise ValueError("vad conf: --%s=%s is not %s" % (name, text, "an integer" if kind is int else "a number"))
    if not 0 <= opts["context"] <= MAX_CONTEXT:
        raise ValueError("vad conf: --vad-frames-context=%d, the window takes 0 .. %d frames on either side" % (opts["context"], MAX_CONTEXT))
    return opts


def frames_of_seconds(sec, shift_sec):
    return int(round(float(sec) / float(shift_sec)))


def runs_of(dec):
    """The maximal runs [a, b) of non-zero entries."""
    out, a = [], None
    for t, d in enumerate(dec):
        if d and a is None:
            a = t
        elif not d and a is not None:
            out.append((a, t))
            a = None
    if a is not None:
        out.append((a, len(dec)))
    return out


def segment(dec, e, min_silence, min_speech, pad, max_segment):
    """-> the segments [a, b) in frames of one recording: ``dec`` its decisions (one per frame), ``e`` its log-energies, the four
    lengths in frames."""
    T = len(dec)
    if max_segment < 2:
        raise ValueError("vad: a longest segment of %d frames (at least 2)" % max_segment)
    merged = []
    for a, b in runs_of(dec):
        if merged and a - merged[-1][1] < min_silence:
            merged[-1][1] = b
        else:
            merged.append([a, b])
    kept = [(a, b) for a, b in merged if b - a >= min_speech]
    padded = [[max(0, a - pad), min(T, b + pad)] for a, b in kept]
    for i in range(len(padded) - 1):
        if padded[i][1] > padded[i + 1][0]:
            padded[i][1] = padded[i + 1][0] = (kept[i][1] + kept[i + 1][0]) // 2
    out = []
    for a, b in padded:
        while b - a > max_segment:
            lo, hi = a + max_segment // 2, a + max_segment
            cut = min(range(lo, hi), key=lambda t: (e[t], t))
            out.append((a, cut))
            a = cut
        out.append((a, b))
    return out
