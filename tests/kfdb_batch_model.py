"""The expected result of a BATCH of key-frame database queries: tests/kfdb_model.py's single members applied in order (the model is the judge; it is
pinned to the reference by tests/golden/kfdb_ref.npz).  After every query the fields of every key frame are recorded, and the situations in which the
order of the queries matters are counted, so that a test can assert that its fixture really contains them."""
import kfdb_model as M


class BatchResult:
    def __init__(self):
        self.results = []            # per query: kfdb_model.Result
        self.fields = []             # per query: {id(kf): (query, words, score)} right after it
        self.count = dict(repeated_qid=0, qid_left_by_earlier_call=0, excluded_then_listed=0, listed_then_excluded=0, stale_score_added=0)


def run_batch(model, kind, queries, min_scores, live):
    """queries: model KFs (mnId the query id; .connected the excluded key frames of a LOOP query); live: every key frame in the database"""
    out = BatchResult()
    before = {id(k): k.fields(kind)[0] for k in live}
    seen_qid, excluded_at, listed_at, scored_in_batch = set(), {}, {}, set()
    for i, q in enumerate(queries):
        if q.mnId in seen_qid:
            out.count["repeated_qid"] += 1
        elif any(before[id(k)] == q.mnId and len(set(k.bow_id.tolist()) & set(q.bow_id.tolist())) for k in live):
            out.count["qid_left_by_earlier_call"] += 1
        seen_qid.add(q.mnId)
        r = model.detect_reloc(q) if kind == 0 else model.detect_loop(q, min_scores[i])
        out.results.append(r)
        out.fields.append({id(k): k.fields(kind) for k in live})
        listed = set(id(k) for k in r.sharing)
        if kind == 1:
            words = set(q.bow_id.tolist())
            for k in q.connected:
                if id(k) not in listed and words & set(k.bow_id.tolist()):
                    excluded_at.setdefault(id(k), []).append(i)
            for k in listed:
                out.count["excluded_then_listed"] += sum(1 for j in excluded_at.get(k, []) if j < i)
                listed_at.setdefault(k, []).append(i)
            for k in q.connected:
                if excluded_at.get(id(k), [None])[-1] == i:
                    out.count["listed_then_excluded"] += sum(1 for j in listed_at.get(id(k), []) if j < i)
        scored_now = set(id(k) for k in r.sharing if k.fields(kind)[1] > r.min_common)
        if kind == 0:
            for _, k in r.scored:
                for k2 in k.best_covisibles(10):
                    if k2.mnRelocQuery == q.mnId and id(k2) not in scored_now and id(k2) in scored_in_batch:
                        out.count["stale_score_added"] += 1
        scored_in_batch |= scored_now
    return out
