"""KeyFrameDatabase.cc restated literally in Python: the inverted file with real per-word lists, the per-key-frame fields, the walks in the reference's
order.  The checker of the device key-frame database (tests/test_kfdb.py); itself pinned against the reference's own member functions by
tests/golden/kfdb_ref.npz.  Scores come from a callable (oracle.OracleVocabulary.score, pinned against the reference's DBoW2); the float steps use
numpy.float32."""
import numpy as np

F32 = np.float32


class KF:
    """The part of ORB_SLAM2::KeyFrame (and, for a relocalisation query, Frame) that KeyFrameDatabase.cc touches."""

    def __init__(self, mnId, bow_id, bow_val):
        self.mnId = int(mnId)
        self.bow_id = np.ascontiguousarray(bow_id, np.uint32)
        self.bow_val = np.ascontiguousarray(bow_val, np.float64)
        # KeyFrame.cc:35 leaves the two scores uninitialised; 0.0f is the canonical initial value
        self.mnLoopQuery, self.mnLoopWords, self.mLoopScore = 0, 0, F32(0)
        self.mnRelocQuery, self.mnRelocWords, self.mRelocScore = 0, 0, F32(0)
        self.connected = []          # GetConnectedKeyFrames()
        self.ordered = []            # GetBestCovisibilityKeyFrames(N) = the first N of these

    def best_covisibles(self, n):
        return self.ordered[:n]

    def fields(self, kind):
        return (self.mnRelocQuery, self.mnRelocWords, self.mRelocScore) if kind == 0 else (self.mnLoopQuery, self.mnLoopWords, self.mLoopScore)


class Result:
    def __init__(self):
        self.sharing = []            # lKFsSharingWords
        self.min_common = 0
        self.scored = []             # lScoreAndMatch: (float32 score, KF)
        self.candidates = []


class ModelDatabase:
    def __init__(self, score):
        self.score = score           # (id1, val1, id2, val2) -> double
        self.inv = {}                # mvInvertedFile: word -> list of KF in add order

    def add(self, kf):
        for w in kf.bow_id:
            self.inv.setdefault(int(w), []).append(kf)

    def erase(self, kf):
        for w in kf.bow_id:
            l = self.inv.get(int(w), [])
            for i, k in enumerate(l):
                if k is kf:
                    del l[i]
                    break

    def clear(self):
        self.inv = {}

    def _score(self, a, b):
        return F32(self.score(a.bow_id, a.bow_val, b.bow_id, b.bow_val))

    def detect_loop(self, kf, min_score):
        r = Result()
        min_score = F32(min_score)
        connected = set(id(k) for k in kf.connected)
        for w in kf.bow_id:
            for k in self.inv.get(int(w), []):
                if k.mnLoopQuery != kf.mnId:
                    k.mnLoopWords = 0
                    if id(k) not in connected:
                        k.mnLoopQuery = kf.mnId
                        r.sharing.append(k)
                k.mnLoopWords += 1
        if not r.sharing:
            return r
        max_common = max(k.mnLoopWords for k in r.sharing)
        r.min_common = int(F32(max_common) * F32(0.8))
        for k in r.sharing:
            if k.mnLoopWords > r.min_common:
                si = self._score(kf, k)
                k.mLoopScore = si
                if si >= min_score:
                    r.scored.append((si, k))
        if not r.scored:
            return r
        acc_list, best_acc = [], min_score
        for si, k in r.scored:
            best_score, acc, best_kf = si, si, k
            for k2 in k.best_covisibles(10):
                if k2.mnLoopQuery == kf.mnId and k2.mnLoopWords > r.min_common:
                    acc = F32(acc + k2.mLoopScore)
                    if k2.mLoopScore > best_score:
                        best_kf, best_score = k2, k2.mLoopScore
            acc_list.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        r.candidates = self._retain(acc_list, best_acc)
        return r

    def detect_reloc(self, frame):
        r = Result()
        for w in frame.bow_id:
            for k in self.inv.get(int(w), []):
                if k.mnRelocQuery != frame.mnId:
                    k.mnRelocWords = 0
                    k.mnRelocQuery = frame.mnId
                    r.sharing.append(k)
                k.mnRelocWords += 1
        if not r.sharing:
            return r
        max_common = max(k.mnRelocWords for k in r.sharing)
        r.min_common = int(F32(max_common) * F32(0.8))
        for k in r.sharing:
            if k.mnRelocWords > r.min_common:
                si = self._score(frame, k)
                k.mRelocScore = si
                r.scored.append((si, k))
        if not r.scored:
            return r
        acc_list, best_acc = [], F32(0)
        for si, k in r.scored:
            best_score, acc, best_kf = si, si, k
            for k2 in k.best_covisibles(10):
                if k2.mnRelocQuery != frame.mnId:
                    continue
                acc = F32(acc + k2.mRelocScore)
                if k2.mRelocScore > best_score:
                    best_kf, best_score = k2, k2.mRelocScore
            acc_list.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        r.candidates = self._retain(acc_list, best_acc)
        return r

    @staticmethod
    def _retain(acc_list, best_acc):
        retain = F32(F32(0.75) * best_acc)
        out, seen = [], set()
        for acc, k in acc_list:
            if acc > retain and id(k) not in seen:
                out.append(k)
                seen.add(id(k))
        return out


def load_golden(path):
    """tests/golden/kfdb_ref.npz (tests/golden/make_golden_kfdb.py) -> (nkf, bows [(ids, vals)], ops [dict], per op: candidates (key-frame indices) or None and
    fields[key frame][kind] = (query, words, float32 score bits))."""
    import json
    g = np.load(path)
    off = g["bow_off"]
    bows = [(g["bow_id"][off[i]:off[i + 1]].copy(), g["bow_val"][off[i]:off[i + 1]].copy()) for i in range(len(off) - 1)]
    ops = json.loads(bytes(g["ops"]).decode())
    nkf = int(g["nkf"])
    res = []
    for i in range(len(ops)):
        cand = [int(c) for c in g["cand"][g["cand_off"][i]:g["cand_off"][i + 1]]] if g["is_query"][i] else None
        fields = [[(int(g["field_query"][i, k, kind]), int(g["field_words"][i, k, kind]), int(g["field_score_bits"][i, k, kind])) for kind in (0, 1)] for k in range(nkf)]
        res.append((cand, fields))
    return nkf, bows, ops, res
