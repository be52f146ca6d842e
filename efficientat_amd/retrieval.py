"""Query-by-example search over audio embeddings: which rows of an index sound like this query.

An `EmbeddingIndex` is a resident matrix of L2-normalised embeddings (N, D) - scene embeddings, one row per recording, or
timestamp embeddings, one row every hop_ms of each recording (efficientat_amd/embeddings.py) - plus host bookkeeping per
row: the file it came from and its time.  Rows of one file are contiguous, so a file is a row range.  `search` returns,
per query, the k rows of largest cosine score in descending order, equal scores by ascending row, optionally leaving out
one file's rows (the query's own).  Normalisation and the fused score + top-k are ``eat_rows_normalize`` and
``eat_embed_search`` (include/eat_search.h, csrc/search.hip): no (Q, N) score matrix exists at any time, and there is no
CPU path - an index without a device keeps books, saves and loads, and refuses to search.

On disk an index is a directory: ``emb.npy`` (N, D) fp32 rows as stored (normalised), ``file.npy`` (N,) int32 file id per
row, ``time_ms.npy`` (N,) float64 (-1 for a scene row), ``names.txt`` one file name per line, ``meta.json``.

storage="q8" keeps a quarter of the bytes: each normalised row as int8 codes and one fp32 scale (``eat_rows_quantize_q8``,
include/eat_search_q8.h), searched by ``eat_embed_search_q8`` with exact integer dot products - up to 64 queries per pass
over the bank instead of 16.  Scores are those of the quantised rows: within about 1e-3 of the cosine at D = 2184 (DESIGN
1.2b).  On disk ``codes.npy`` (N, D) int8 and ``scale.npy`` (N,) float32 take the place of ``emb.npy``, and ``meta.json`` has
version 2 and one more entry, "storage": "q8".  The fp32 index is the default and writes what it always wrote.
"""
import json
import os

import numpy as np
import torch

from . import _lib, ops

VERSION = 1
VERSION_Q8 = 2               # meta.json of a q8 index: META_KEYS and "storage"
STORAGES = ("fp32", "q8")
KINDS = ("scene", "timestamps")
META_KEYS = ("version", "D", "kind", "model_name", "layers", "clip_seconds", "hop_ms", "width_ms")


def _default_meta(D):
    return {"version": VERSION, "D": int(D), "kind": "scene", "model_name": None, "layers": None, "clip_seconds": None,
            "hop_ms": None, "width_ms": None}


class EmbeddingIndex:
    """D       embedding size
    device  where the bank lives; None: on the CPU, for bookkeeping, `save` and `load` only - `add` then stores the rows AS
            GIVEN (rows downloaded from another index; nothing normalises on the CPU) and `search` raises EatHipError
    meta    entries of `META_KEYS` to record (kind, model_name, layers, clip_seconds, hop_ms, width_ms)
    storage "fp32": the rows as they are; "q8": int8 codes and one scale per row - rows are quantised by a kernel, so without
            a device a q8 index loads, saves and keeps books, and `add` raises EatHipError like `search`"""

    def __init__(self, D, device=None, meta=None, storage="fp32"):
        if int(D) < 1:
            raise ValueError(f"EmbeddingIndex: need D >= 1 (got {D})")
        if storage not in STORAGES:
            raise ValueError(f"EmbeddingIndex: storage must be one of {STORAGES} (got {storage!r})")
        if storage == "q8" and int(D) > ops.SEARCH_Q8_MAX_D:
            raise ValueError(f"EmbeddingIndex: q8 storage needs D <= {ops.SEARCH_Q8_MAX_D} (got {D})")
        self.storage = storage
        self.D = int(D)
        self.device = None if device is None else torch.device(device)
        if self.device is not None and self.device.type != "cuda":
            raise ValueError(f"EmbeddingIndex: device must be a GPU or None (got {self.device})")
        if self.device is not None and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        version = VERSION_Q8 if storage == "q8" else VERSION
        self.meta = dict(_default_meta(self.D), version=version)
        for key, value in (meta or {}).items():
            if key not in META_KEYS:
                raise ValueError(f"EmbeddingIndex: unknown meta entry '{key}' (known: {', '.join(META_KEYS)})")
            self.meta[key] = value
        if self.meta["version"] != version or self.meta["D"] != self.D or self.meta["kind"] not in KINDS:
            raise ValueError(f"EmbeddingIndex: meta needs version = {version}, D = {self.D} and kind in {KINDS} (got {self.meta})")
        self.names = []
        self._ranges = {}                                        # name -> (lo, hi)
        self._file = np.zeros(0, dtype=np.int32)
        self._time = np.zeros(0, dtype=np.float64)
        self._bank = self._codes = self._scale = None             # fp32: _bank (cap, D); q8: _codes (cap, ld) int8, _scale (cap,)
        if storage == "q8":
            self._codes = torch.empty((0, ops.q8_ld(self.D)), dtype=torch.int8, device=self.device or "cpu")
            self._scale = torch.empty((0,), dtype=torch.float32, device=self.device or "cpu")
        else:
            self._bank = torch.empty((0, self.D), dtype=torch.float32, device=self.device or "cpu")
        self._n = 0
        self._seg = None                                         # `find`: (F + 1,) int32 file bounds on the device; None: rebuild
        self._uniform = None                                     # `find`: every file's times step by hop_ms; None: not checked yet

    # -- bookkeeping -----------------------------------------------------------------------------------------------------
    def __len__(self):
        return self._n

    @property
    def bank(self):
        """The rows as stored, (N, D) fp32 on the index's device (a view of the resident buffer); fp32 storage only."""
        if self.storage != "fp32":
            raise ValueError(f"EmbeddingIndex: an index of storage '{self.storage}' has no fp32 bank (see `codes` and `scales`)")
        return self._bank[:self._n]

    @property
    def codes(self):
        """q8 storage: the codes as stored, (N, ld) int8 with ld = D rounded up to 16 and zeros from column D on (a view)."""
        if self.storage != "q8":
            raise ValueError(f"EmbeddingIndex: an index of storage '{self.storage}' has no codes (see `bank`)")
        return self._codes[:self._n]

    @property
    def scales(self):
        """q8 storage: (N,) fp32, row n stands for scales[n] * codes[n, :D] (a view)."""
        if self.storage != "q8":
            raise ValueError(f"EmbeddingIndex: an index of storage '{self.storage}' has no scales (see `bank`)")
        return self._scale[:self._n]

    @property
    def file_ids(self):
        return self._file

    @property
    def time_ms(self):
        return self._time

    def row_range(self, name):
        if name not in self._ranges:
            raise ValueError(f"EmbeddingIndex: no file named '{name}' in the index")
        return self._ranges[name]

    def add(self, emb, name, times_ms=None):
        """One file's rows: emb (n >= 1, D), times_ms None (scene rows) or (n,) >= 0 -> the row range (lo, hi).  On a device
        the rows are L2-normalised by `ops.rows_normalize` straight into the resident bank, which grows by doubling; a q8
        index normalises and quantises them in one launch of `ops.rows_quantize_q8`, straight into its codes and scales."""
        name = str(name)
        if name in self._ranges:
            raise ValueError(f"EmbeddingIndex: a file named '{name}' is in the index already")
        if name == "" or "\n" in name or "\r" in name:
            raise ValueError(f"EmbeddingIndex: a file name must be one non-empty line (got {name!r})")
        emb = torch.as_tensor(emb)
        if emb.dim() == 1:
            emb = emb.unsqueeze(0)
        if emb.dim() != 2 or emb.shape[0] < 1 or emb.shape[1] != self.D:
            raise ValueError(f"EmbeddingIndex: rows of '{name}' must be (n >= 1, {self.D}) (got {tuple(emb.shape)})")
        n = emb.shape[0]
        if times_ms is None:
            times = np.full(n, -1.0, dtype=np.float64)
        else:
            times = np.asarray(times_ms, dtype=np.float64).reshape(-1)
            if times.shape != (n,) or not bool(np.isfinite(times).all()) or bool((times < 0).any()):
                raise ValueError(f"EmbeddingIndex: times_ms of '{name}' must be {n} finite values >= 0")
        kind = "scene" if times_ms is None else "timestamps"
        if self._n > 0 and kind != self.meta["kind"]:
            raise ValueError(f"EmbeddingIndex: '{name}' brings {kind} rows into an index of {self.meta['kind']} rows")
        if self._n + n > 2 ** 31 - 1:
            raise ValueError("EmbeddingIndex: more than 2^31 - 1 rows")
        if self.storage == "q8" and self.device is None:
            raise _lib.EatHipError("EmbeddingIndex.add needs a q8 index on a GPU: rows are quantised by a kernel and "
                                   "efficientat_amd has no CPU path (load it with device='cuda')")
        self.meta["kind"] = kind
        lo, hi = self._n, self._n + n
        if self.storage == "q8":
            self._add_q8(emb, lo, hi)
        else:
            self._add_fp32(emb, lo, hi)
        self._file = np.concatenate((self._file, np.full(n, len(self.names), dtype=np.int32)))
        self._time = np.concatenate((self._time, times))
        self.names.append(name)
        self._ranges[name] = (lo, hi)
        self._n = hi
        self._seg = self._uniform = None
        return lo, hi

    def _add_fp32(self, emb, lo, hi):
        if hi > self._bank.shape[0]:
            grown = torch.empty((max(hi, 2 * self._bank.shape[0], 64), self.D), dtype=torch.float32, device=self._bank.device)
            grown[:lo] = self._bank[:lo]
            self._bank = grown
        emb = emb.to(device=self._bank.device, dtype=torch.float32).contiguous()
        if self.device is None:
            self._bank[lo:hi] = emb
        else:
            with torch.cuda.device(self.device):
                ops.rows_normalize(emb, out=self._bank[lo:hi])

    def _add_q8(self, emb, lo, hi, normalize=True):
        cap = self._codes.shape[0]
        if hi > cap:
            cap = max(hi, 2 * cap, 64)
            codes = torch.empty((cap, self._codes.shape[1]), dtype=torch.int8, device=self.device)
            scale = torch.empty((cap,), dtype=torch.float32, device=self.device)
            codes[:lo] = self._codes[:lo]
            scale[:lo] = self._scale[:lo]
            self._codes, self._scale = codes, scale
        with torch.cuda.device(self.device):
            ops.rows_quantize_q8(emb.to(device=self.device, dtype=torch.float32).contiguous(), normalize=normalize,
                                 codes=self._codes[lo:hi], scale=self._scale[lo:hi])

    def quantized(self):
        """The q8 index of this fp32 index's stored rows on the same device: they are normalised already, so they are
        quantised as they are, and the books are copied."""
        if self.storage != "fp32" or self.device is None:
            raise ValueError("EmbeddingIndex.quantized: needs an fp32 index on a GPU")
        meta = {key: value for key, value in self.meta.items() if key != "version"}
        out = EmbeddingIndex(self.D, device=self.device, meta=meta, storage="q8")
        if self._n:
            out._add_q8(self.bank, 0, self._n, normalize=False)
        out._n = self._n
        out._file, out._time, out.names, out._ranges = self._file.copy(), self._time.copy(), list(self.names), dict(self._ranges)
        return out

    # -- search ----------------------------------------------------------------------------------------------------------
    def check_extractor(self, extractor):
        """ValueError unless the extractor's (D, layers, clip_seconds) are those the index was built with (entries that meta
        does not record - None - are not compared)."""
        got = {"D": int(extractor.scene_embedding_size), "layers": [int(i) for i in extractor.layers],
               "clip_seconds": float(extractor.clip_seconds)}
        for key, value in got.items():
            want = self.meta[key]
            if want is not None and (list(want) if key == "layers" else want) != value:
                raise ValueError(f"EmbeddingIndex: the index was built with {key} = {want}, the extractor has {key} = {value}: "
                                 f"their embeddings do not compare")

    def search(self, queries, k, exclude=None, extractor=None):
        """queries (Q, D), k -> (score (Q, k) fp32, index (Q, k) int32) on the device: the k rows of largest cosine score per
        query in descending order, equal scores by ascending row, (-inf, -1) where fewer than k rows are eligible.
        exclude: per query, None or the name of a file whose rows are not eligible.  The queries are normalised by the
        kernel that normalised the bank (a q8 index quantises them as it quantised its rows, and the scores are those of the
        quantised vectors).  extractor: where the queries come from, checked by `check_extractor`."""
        if self.device is None:
            raise _lib.EatHipError("EmbeddingIndex.search needs the index on a GPU: efficientat_amd has no CPU path "
                                   "(load it with device='cuda')")
        if extractor is not None:
            self.check_extractor(extractor)
        if self._n < 1:
            raise ValueError("EmbeddingIndex: the index is empty")
        queries = torch.as_tensor(queries)
        if queries.dim() == 1:
            queries = queries.unsqueeze(0)
        if queries.dim() != 2 or queries.shape[1] != self.D or queries.shape[0] < 1:
            raise ValueError(f"EmbeddingIndex: queries must be (Q >= 1, {self.D}) (got {tuple(queries.shape)})")
        Q = queries.shape[0]
        skip = None
        if exclude is not None:
            exclude = [exclude] * Q if isinstance(exclude, str) else list(exclude)
            if len(exclude) != Q:
                raise ValueError(f"EmbeddingIndex: exclude must hold one name or None per query ({Q}), got {len(exclude)}")
            skip = [(0, 0) if name is None else self.row_range(name) for name in exclude]
        with torch.cuda.device(self.device):
            queries = queries.to(device=self.device, dtype=torch.float32).contiguous()
            if self.storage == "q8":
                qcodes, qscale = ops.rows_quantize_q8(queries, normalize=True)
                return ops.embed_search_q8(self.codes, self.scales, self.D, qcodes, qscale, k, skip)
            return ops.embed_search(self.bank, ops.rows_normalize(queries), k, skip)

    # -- occurrences -----------------------------------------------------------------------------------------------------
    def _check_times(self):
        """ValueError unless every file's time_ms is an arithmetic progression of step meta["hop_ms"] (checked once, on the
        host, until the next `add`): a sequence of query rows at that hop then lines up with consecutive rows of a file."""
        if self._uniform is None:
            hop = self.meta["hop_ms"]
            if hop is None or not float(hop) > 0:
                raise ValueError(f"EmbeddingIndex.find: the index records no hop_ms (meta hop_ms = {hop!r}): pass it in meta")
            steps = np.diff(self._time)
            inside = np.diff(self._file) == 0
            self._uniform = bool((np.abs(steps[inside] - float(hop)) <= 1e-6 * float(hop)).all())
        if not self._uniform:
            raise ValueError(f"EmbeddingIndex.find: the times of a file do not step by hop_ms = {self.meta['hop_ms']}: rows of "
                             f"a sequence match must be evenly spaced")

    def find(self, query_rows, k, min_separation_rows=None, min_score=None, exclude=None, extractor=None, allow_q8=False):
        """Where in the files of a timestamp index does the clip occur whose timestamp embeddings are query_rows (L, D), in
        time order at the index's hop_ms -> (score (k,) fp32, row (k,) int32) on the device: distinct occurrences, best
        first, (-inf, -1) where there are fewer than k.  The score of a start row is the mean cosine of the L query rows with
        the L rows from it on, all within one file; a start row is an occurrence when no other start row of its file within
        min_separation_rows (default max(L, ceil(width_ms / hop_ms)): occurrences do not overlap) scores higher - local-maximum
        peak picking (`ops.embed_match`, include/eat_match.h).  min_score: occurrences below it are left out.  exclude:
        None or the name of a file whose rows are no start rows.  An index of kind "timestamps" on a GPU only, and an fp32
        one unless allow_q8: then a q8 index quantises the query rows as it quantised its own (`ops.rows_quantize_q8`) and
        matches the codes (`ops.embed_match_q8`, include/eat_match_q8.h).  The scores are then those of the codes: a mean of
        q8 scores, on the scale of the `search` scores of the same index, not the fp32 cosines.  On an fp32 index allow_q8
        changes nothing."""
        if self.storage != "fp32" and not allow_q8:
            raise ValueError(f"EmbeddingIndex.find: a sequence match needs the fp32 index (this one has storage '{self.storage}'; "
                             f"allow_q8=True matches the codes instead)")
        if self.meta["kind"] != "timestamps":
            raise ValueError(f"EmbeddingIndex.find: occurrences are found in an index of kind 'timestamps' (this one is "
                             f"'{self.meta['kind']}'; see `search`)")
        if self.device is None:
            raise _lib.EatHipError("EmbeddingIndex.find needs the index on a GPU: efficientat_amd has no CPU path "
                                   "(load it with device='cuda')")
        if extractor is not None:
            self.check_extractor(extractor)
        if self._n < 1:
            raise ValueError("EmbeddingIndex: the index is empty")
        query_rows = torch.as_tensor(query_rows)
        if query_rows.dim() == 1:
            query_rows = query_rows.unsqueeze(0)
        if query_rows.dim() != 2 or query_rows.shape[1] != self.D or query_rows.shape[0] < 1:
            raise ValueError(f"EmbeddingIndex.find: query_rows must be (L >= 1, {self.D}) (got {tuple(query_rows.shape)})")
        self._check_times()
        L = query_rows.shape[0]
        if min_separation_rows is None:
            min_separation_rows = max(L, int(np.ceil(float(self.meta["width_ms"] or 0.0) / float(self.meta["hop_ms"]))))
        if int(min_separation_rows) != min_separation_rows or min_separation_rows < 0:
            raise ValueError(f"EmbeddingIndex.find: min_separation_rows must be an integer >= 0 (got {min_separation_rows!r})")
        skip = None if exclude is None else self.row_range(exclude)
        with torch.cuda.device(self.device):
            if self._seg is None:
                bounds = [0] + [self._ranges[name][1] for name in self.names]
                self._seg = torch.tensor(bounds, dtype=torch.int32).to(self.device)
            query_rows = query_rows.to(device=self.device, dtype=torch.float32).contiguous()
            min_score = float("-inf") if min_score is None else min_score
            if self.storage == "q8":
                qcodes, qscale = ops.rows_quantize_q8(query_rows, normalize=True)
                return ops.embed_match_q8(self.codes, self.scales, self.D, self._seg, qcodes, qscale, k, int(min_separation_rows),
                                          min_score, skip)
            return ops.embed_match(self.bank, self._seg, ops.rows_normalize(query_rows), k, int(min_separation_rows), min_score, skip)

    def find_recordings(self, extractor, waves, k, min_separation_rows=None, min_score=None, exclude=None, allow_q8=False):
        """`find` for each query clip of `waves` (what `EmbeddingExtractor.timestamp_embeddings` takes), embedded at the
        index's hop_ms and width_ms -> per clip (score (k,), row (k,), L): L, the clip's rows, is what `hits` needs.
        exclude: None, or per clip None or a file name.  allow_q8: as in `find`."""
        self.check_extractor(extractor)
        if self.meta["hop_ms"] is None or self.meta["width_ms"] is None:
            raise ValueError("EmbeddingIndex.find_recordings: the index records no hop_ms / width_ms to embed the queries at")
        clips = extractor.timestamp_embeddings(waves, hop_ms=self.meta["hop_ms"], width_ms=self.meta["width_ms"])
        exclude = [None] * len(clips) if exclude is None else list(exclude)
        if len(exclude) != len(clips):
            raise ValueError(f"EmbeddingIndex.find_recordings: exclude must hold one name or None per clip ({len(clips)}), "
                             f"got {len(exclude)}")
        return [self.find(emb, k, min_separation_rows, min_score, name, allow_q8=allow_q8) + (emb.shape[0],)
                for (emb, _), name in zip(clips, exclude)]

    def hits(self, score, index, query_rows=None):
        """(score, index) of `search` -> per query a host list of {"name", "time_ms" (None for a scene row), "row", "score"},
        best first, without the -1 slots.  query_rows = L: (score, index) are the (k,) outputs of `find` for a clip of L rows;
        the result is that clip's one list, and each place gains "end_ms" = time_ms + L hop_ms."""
        score, index = torch.as_tensor(score).cpu().numpy(), torch.as_tensor(index).cpu().numpy()
        if query_rows is not None:
            if score.ndim != 1:
                raise ValueError(f"EmbeddingIndex.hits: with query_rows, score and index are the (k,) outputs of `find` (got {score.shape})")
            span = int(query_rows) * float(self.meta["hop_ms"])
            (found,) = self.hits(score[None], index[None])
            return [dict(h, end_ms=h["time_ms"] + span) for h in found]
        if score.shape != index.shape or score.ndim != 2:
            raise ValueError(f"EmbeddingIndex.hits: score and index must share one (Q, k) shape (got {score.shape}, {index.shape})")
        if bool(((index < -1) | (index >= self._n)).any()):
            raise ValueError(f"EmbeddingIndex.hits: a row index outside [-1, {self._n})")
        out = []
        for s_row, i_row in zip(score, index):
            found = []
            for s, i in zip(s_row, i_row):
                if i >= 0:
                    t = float(self._time[i])
                    found.append({"name": self.names[self._file[i]], "time_ms": None if t < 0 else t, "row": int(i), "score": float(s)})
            out.append(found)
        return out

    # -- disk ------------------------------------------------------------------------------------------------------------
    def save(self, path):
        os.makedirs(path, exist_ok=True)
        if self.storage == "q8":
            np.save(os.path.join(path, "codes.npy"), np.ascontiguousarray(self.codes[:, :self.D].cpu().numpy()))
            np.save(os.path.join(path, "scale.npy"), self.scales.cpu().numpy())
        else:
            np.save(os.path.join(path, "emb.npy"), self.bank.cpu().numpy())
        np.save(os.path.join(path, "file.npy"), self._file)
        np.save(os.path.join(path, "time_ms.npy"), self._time)
        with open(os.path.join(path, "names.txt"), "w") as f:
            f.write("".join(name + "\n" for name in self.names))
        with open(os.path.join(path, "meta.json"), "w") as f:
            meta = {key: self.meta[key] for key in META_KEYS}
            if self.storage == "q8":
                meta["storage"] = "q8"
            json.dump(meta, f, indent=1)
            f.write("\n")

    @classmethod
    def load(cls, path, device=None):
        """The index that `save` wrote into the directory `path`, its rows as stored (not normalised again: a search gives
        the bits it gave before).  ValueError, naming the path, for anything that `save` could not have written."""
        def bad(what):
            return ValueError(f"EmbeddingIndex.load: {path}: {what}")

        def read(name, reader):
            full = os.path.join(path, name)
            if not os.path.isfile(full):
                raise bad(f"{name} is missing")
            try:
                return reader(full)
            except (ValueError, OSError, EOFError, UnicodeDecodeError) as e:
                raise bad(f"{name} is unreadable ({e})") from None

        def text(full):
            with open(full) as f:
                return f.read()

        try:
            meta = json.loads(read("meta.json", text))
        except json.JSONDecodeError as e:
            raise bad(f"meta.json is not JSON ({e})") from None
        if isinstance(meta, dict) and meta.get("version") == VERSION_Q8:
            if set(meta) != set(META_KEYS) | {"storage"}:
                raise bad(f"meta.json of version {VERSION_Q8} must hold exactly the entries {', '.join(META_KEYS)}, storage")
            if meta["storage"] != "q8":
                raise bad(f"meta.json of version {VERSION_Q8} needs storage = 'q8' (got {meta['storage']!r})")
            meta = {key: meta[key] for key in META_KEYS}
            return cls._load_rest(path, device, meta, "q8", bad, read, text)
        if not isinstance(meta, dict) or set(meta) != set(META_KEYS):
            raise bad(f"meta.json must hold exactly the entries {', '.join(META_KEYS)}")
        if meta["version"] != VERSION:
            raise bad(f"meta.json has version {meta['version']!r}, this code reads version {VERSION}")
        return cls._load_rest(path, device, meta, "fp32", bad, read, text)

    @classmethod
    def _load_rest(cls, path, device, meta, storage, bad, read, text):
        """`load` past meta.json's entries and version: the arrays, and the checks on them."""
        if not isinstance(meta["D"], int) or isinstance(meta["D"], bool) or meta["D"] < 1 or meta["kind"] not in KINDS:
            raise bad(f"meta.json needs an integer D >= 1 and kind in {KINDS} (got D = {meta['D']!r}, kind = {meta['kind']!r})")
        D = meta["D"]
        if storage == "q8":
            if D > ops.SEARCH_Q8_MAX_D:
                raise bad(f"meta.json of a q8 index needs D <= {ops.SEARCH_Q8_MAX_D} (got {D})")
            emb = read("codes.npy", lambda p: np.load(p, allow_pickle=False))
            scale = read("scale.npy", lambda p: np.load(p, allow_pickle=False))
        else:
            emb = read("emb.npy", lambda p: np.load(p, allow_pickle=False))
        file = read("file.npy", lambda p: np.load(p, allow_pickle=False))
        time = read("time_ms.npy", lambda p: np.load(p, allow_pickle=False))
        names = read("names.txt", text).split("\n")
        if names[-1] != "":
            raise bad("names.txt does not end with a newline")
        names = names[:-1]
        if storage == "q8":
            if emb.ndim != 2 or emb.shape[1] != D or emb.dtype != np.int8:
                raise bad(f"codes.npy must be (N, {D}) int8 (got {emb.shape} {emb.dtype})")
            if scale.shape != (emb.shape[0],) or scale.dtype != np.float32:
                raise bad(f"scale.npy must be ({emb.shape[0]},) float32 (got {scale.shape} {scale.dtype})")
        elif emb.ndim != 2 or emb.shape[1] != D or emb.dtype != np.float32:
            raise bad(f"emb.npy must be (N, {D}) float32 (got {emb.shape} {emb.dtype})")
        N = emb.shape[0]
        if file.shape != (N,) or file.dtype != np.int32:
            raise bad(f"file.npy must be ({N},) int32 (got {file.shape} {file.dtype})")
        if time.shape != (N,) or time.dtype != np.float64:
            raise bad(f"time_ms.npy must be ({N},) float64 (got {time.shape} {time.dtype})")
        if storage == "q8":
            if bool((emb == -128).any()):
                raise bad("codes.npy holds a code outside [-127, 127]")
            if not bool(np.isfinite(scale).all()) or bool((scale < 0).any()):
                raise bad("scale.npy holds a scale that is negative or not finite")
            if bool(((scale == 0)[:, None] & (emb != 0)).any()):
                raise bad("codes.npy holds non-zero codes in a row whose scale is 0")
        elif not bool(np.isfinite(emb).all()):
            raise bad("emb.npy holds a value that is not finite")
        if len(set(names)) != len(names) or any(name == "" for name in names):
            raise bad("names.txt holds an empty or a repeated name")
        if bool(((file < 0) | (file >= len(names))).any()):
            raise bad(f"file.npy holds a file id outside [0, {len(names)})")
        # every file has rows, and they are contiguous: the ids go 0, .., 0, 1, .., 1, 2, ..
        steps = np.diff(file.astype(np.int64))
        if (N == 0) != (len(names) == 0) or (N > 0 and (file[0] != 0 or file[-1] != len(names) - 1
                                                        or not bool(((steps == 0) | (steps == 1)).all()))):
            raise bad("the rows of each file must be contiguous, in the order of names.txt, and every file must have rows")
        scene = meta["kind"] == "scene"
        if not bool(np.isfinite(time).all()) or (scene and not bool((time == -1.0).all())) or (not scene and bool((time < 0).any())):
            raise bad(f"time_ms.npy must hold -1 for every row of a scene index and times >= 0 otherwise (kind = {meta['kind']})")
        index = cls(D, device=device, meta=meta, storage=storage)
        if storage == "q8":
            padded = np.zeros((N, ops.q8_ld(D)), dtype=np.int8)
            padded[:, :D] = emb
            index._codes = torch.from_numpy(padded).to(index.device or "cpu")
            index._scale = torch.from_numpy(scale.copy()).to(index.device or "cpu")
        else:
            index._bank = torch.from_numpy(np.ascontiguousarray(emb)).to(index.device or "cpu")
        index._n = N
        index._file, index._time, index.names = file.copy(), time.copy(), names
        bounds = np.flatnonzero(np.diff(file)) + 1 if N else np.zeros(0, dtype=np.int64)
        los = [0] + [int(b) for b in bounds]
        his = [int(b) for b in bounds] + [N]
        index._ranges = {name: (lo, hi) for name, lo, hi in zip(names, los, his)}
        return index

    # -- from audio ------------------------------------------------------------------------------------------------------
    @classmethod
    def from_recordings(cls, extractor, waves, names, timestamps=False, hop_ms=50.0, width_ms=160.0, model_name=None,
                        storage="fp32"):
        """An index on the extractor's device of the recordings `waves` (what `EmbeddingExtractor.scene_embeddings` takes)
        named `names`, of the given storage: their scene embeddings, or with timestamps=True their timestamp embeddings (hop_ms,
        width_ms).  A
        scene query searched in a timestamp index finds where the query occurs: choose width_ms near the query's length."""
        names = [str(n) for n in names]
        if len(names) != len(waves):
            raise ValueError(f"EmbeddingIndex.from_recordings: {len(waves)} recordings, {len(names)} names")
        meta = {"kind": "timestamps" if timestamps else "scene", "model_name": model_name,
                "layers": [int(i) for i in extractor.layers], "clip_seconds": float(extractor.clip_seconds),
                "hop_ms": float(hop_ms) if timestamps else None, "width_ms": float(width_ms) if timestamps else None}
        index = cls(extractor.scene_embedding_size, device=extractor.device, meta=meta, storage=storage)
        if timestamps:
            for name, (emb, t_ms) in zip(names, extractor.timestamp_embeddings(waves, hop_ms=hop_ms, width_ms=width_ms)):
                index.add(emb, name, t_ms)
        else:
            for name, emb in zip(names, extractor.scene_embeddings(waves)):
                index.add(emb, name)
        return index
