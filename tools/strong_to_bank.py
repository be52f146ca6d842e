"""WAV files + a strong-label table -> a decoded strong-label bank directory (waves.npy, lengths.npy, names.txt, classes.txt,
events.npy, event_offsets.npy and, with a weak table, strong.npy: efficientat_amd/sed.py).

    python tools/strong_to_bank.py AUDIO_DIR ANNOTATIONS.tsv OUT [--classes classes.txt] [--float32] [--weak_tsv WEAK.tsv]

ANNOTATIONS.tsv: tab-separated `filename onset offset event_label` rows in seconds, as DESED and AudioSet-strong ship them;
a header row (one whose onset is not a number) is optional.  The clips are the WAV files of AUDIO_DIR in sorted order; a file
without rows is a clip without events, a row naming no file of AUDIO_DIR is an error.  Decoding is scipy.io.wavfile;
down-mix and resampling to 32 kHz are `efficientat_amd.audio_io.load_audio`'s, on the host.  Classes: the sorted label names,
or the lines of --classes in their order (a label outside it is an error).  An onset is floored to a sample, an offset
ceiled, both are clipped to the clip's length; an event that becomes empty is dropped and the drops are reported.
--weak_tsv WEAK.tsv: tab-separated `filename event_labels` rows with the labels separated by commas, as DESED's weak.tsv; a
header row (`filename	event_labels`) is optional.  The files it names become WEAKLY labelled clips: each tag is stored as an
event that spans the whole clip, and strong.npy (written only with this option) holds 0 for them and 1 for the others.  A
file named in both tables is an error; one named in neither stays a strong clip without events."""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SAMPLE_RATE = 32000
I16_SCALE = 32767.0                                     # efficientat_amd.input_pipeline.I16_SCALE


def read_table(path):
    """-> [(filename, onset_s, offset_s, label)] of a tab-separated table; an optional header row is skipped."""
    rows = []
    with open(path) as f:
        for ln, line in enumerate(f):
            line = line.rstrip("\r\n")
            if not line.strip():
                continue
            cells = line.split("\t")
            if len(cells) < 4:
                raise ValueError(f"{path}:{ln + 1}: expected `filename onset offset event_label`, got {len(cells)} cells")
            name, on, off, label = (c.strip() for c in cells[:4])
            try:
                on, off = float(on), float(off)
            except ValueError:
                if not rows and ln == 0:
                    continue                                                   # the header row
                raise ValueError(f"{path}:{ln + 1}: onset / offset are not numbers") from None
            if not label or not math.isfinite(on) or not math.isfinite(off):
                raise ValueError(f"{path}:{ln + 1}: an empty label or a non-finite time")
            rows.append((name, on, off, label))
    return rows


def read_weak_table(path):
    """-> [(filename, [label, ...])] of a tab-separated `filename event_labels` table; an optional header row is skipped."""
    rows = []
    with open(path) as f:
        for ln, line in enumerate(f):
            line = line.rstrip("\r\n")
            if not line.strip():
                continue
            cells = [c.strip() for c in line.split("\t")]
            if len(cells) < 2:
                raise ValueError(f"{path}:{ln + 1}: expected `filename event_labels`, got {len(cells)} cell")
            if ln == 0 and not rows and cells[0].lower() == "filename":
                continue                                                       # the header row
            labels = [t.strip() for t in cells[1].split(",")]
            if not cells[0] or not labels or any(not t for t in labels):
                raise ValueError(f"{path}:{ln + 1}: an empty file name or label")
            rows.append((cells[0], labels))
    return rows


def convert(audio_dir, table, out, classes_file=None, float32=False, weak_table=None):
    """-> (clips, events kept, events dropped).  weak_table: a `filename event_labels` table of weakly labelled clips."""
    from efficientat_amd.audio_io import load_audio
    files = sorted(f for f in os.listdir(audio_dir) if f.lower().endswith(".wav"))
    if not files:
        raise ValueError(f"{audio_dir}: no WAV files")
    rows = read_table(table)
    stray = sorted({r[0] for r in rows} - set(files))
    if stray:
        raise ValueError(f"{table}: {len(stray)} file names are not in {audio_dir}, e.g. {stray[0]}")
    weak_rows = [] if weak_table is None else read_weak_table(weak_table)
    tags = {}
    for name, labels in weak_rows:
        tags.setdefault(name, []).extend(labels)
    stray = sorted(set(tags) - set(files))
    if stray:
        raise ValueError(f"{weak_table}: {len(stray)} file names are not in {audio_dir}, e.g. {stray[0]}")
    both = sorted(set(tags) & {r[0] for r in rows})
    if both:
        raise ValueError(f"{weak_table}: {len(both)} files are named in both tables, e.g. {both[0]}")
    weak_labels = {t for labels in tags.values() for t in labels}
    if classes_file is not None:
        with open(classes_file) as f:
            classes = f.read().splitlines()
        unknown = sorted({r[3] for r in rows} - set(classes))
        if unknown:
            raise ValueError(f"{table}: label {unknown[0]!r} is not in {classes_file}")
        unknown = sorted(weak_labels - set(classes))
        if unknown:
            raise ValueError(f"{weak_table}: label {unknown[0]!r} is not in {classes_file}")
    else:
        classes = sorted({r[3] for r in rows} | weak_labels)
    if not classes or len(set(classes)) != len(classes):
        raise ValueError("no classes, or a class named twice")
    cls_of = {c: i for i, c in enumerate(classes)}
    by_file = {}
    for name, on, off, label in rows:
        by_file.setdefault(name, []).append((cls_of[label], on, off))

    os.makedirs(out, exist_ok=True)
    waves, lengths, events, eo, dropped, strong = [], [], [], [0], 0, []
    for name in files:
        x, _ = load_audio(os.path.join(audio_dir, name), sr=SAMPLE_RATE, mono=True)
        n = x.shape[0]
        if n < 1:
            raise ValueError(f"{name}: no audio frames")
        waves.append(x if float32 else np.rint(np.clip(x, -1.0, 1.0) * I16_SCALE).astype(np.int16))
        lengths.append(n)
        strong.append(0 if name in tags else 1)
        mine = [(c, 0, n) for c in sorted({cls_of[t] for t in tags.get(name, [])})]    # a weak clip's tags span the whole clip
        for c, on, off in by_file.get(name, []):
            a = min(max(int(math.floor(on * SAMPLE_RATE)), 0), n)
            b = min(max(int(math.ceil(off * SAMPLE_RATE)), 0), n)
            if a < b:
                mine.append((c, a, b))
            else:
                dropped += 1
        events.extend(sorted(mine))
        eo.append(len(events))
    np.save(os.path.join(out, "waves.npy"), np.concatenate(waves))
    np.save(os.path.join(out, "lengths.npy"), np.asarray(lengths, dtype=np.int64))
    np.save(os.path.join(out, "events.npy"), np.asarray(events, dtype=np.int32).reshape(-1, 3))
    np.save(os.path.join(out, "event_offsets.npy"), np.asarray(eo, dtype=np.int64))
    if weak_table is not None:
        np.save(os.path.join(out, "strong.npy"), np.asarray(strong, dtype=np.uint8))
    for fname, lines in (("names.txt", files), ("classes.txt", classes)):
        with open(os.path.join(out, fname), "w") as g:
            g.write("\n".join(lines) + "\n")
    return len(files), len(events), dropped


if __name__ == "__main__":
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("audio_dir")
    p.add_argument("annotations")
    p.add_argument("out")
    p.add_argument("--classes", default=None, help="file with one class name per line, in index order (default: sorted labels)")
    p.add_argument("--float32", action="store_true", help="store fp32 waveforms (default: int16)")
    p.add_argument("--weak_tsv", default=None, help="`filename event_labels` table of weakly labelled clips (writes strong.npy)")
    a = p.parse_args()
    n, kept, dropped = convert(a.audio_dir, a.annotations, a.out, a.classes, a.float32, a.weak_tsv)
    print(f"{n} clips, {kept} events -> {a.out}" + (f" ({dropped} events dropped: empty after clipping to their clip)" if dropped else ""))
