"""TEST INFRASTRUCTURE ONLY: the rule of the three kernels of csrc/track_lifecycle.hip (include/centernet_gfx950.h: cnl_track_lifecycle_i32,
cnl_track_lifecycle_emit_f64) restated in numpy on plain arrays — the track life cycle of a TrackerBank step at a fixed capacity of
max_tracks rows per stream.  tests/test_lifecycle_host.py holds it equal to the host path's `_track_host.life_cycle` + `Track`.

State (`new_state`): per row of the pooled table (C = S * max_tracks rows, the live ones first, zeros behind) track_id int64, state /
birth_age / inactive_age / label int32, box float64 [C, 4] (the reported box); trk_off int32 [S + 1]; next_track_id int64 [S]; status int32
[S, 2] (sticky: association code | overflow bit, step of the first event).
A stream's association (`assoc[s]`, what its record holds): dict(status, matches [(detection row, track)], low_matches [(ORIGINAL detection
index, track)], unmatched_dets [rows], det_index [n]).
"""
import numpy as np

UNCONFIRMED, ACTIVE, INACTIVE, TO_DELETE = 1, 2, 3, 4
OVERFLOW = 1 << 16
ROW_FIELDS = ("track_id", "state", "birth_age", "inactive_age", "label")


def new_state(S, M):
    C = S * M
    return dict(track_id=np.zeros(C, np.int64), state=np.zeros(C, np.int32), birth_age=np.zeros(C, np.int32), inactive_age=np.zeros(C, np.int32),
                label=np.zeros(C, np.int32), box=np.zeros((C, 4), np.float64), trk_off=np.zeros(S + 1, np.int32),
                next_track_id=np.zeros(S, np.int64), status=np.zeros((S, 2), np.int32))


def lifecycle(st, assoc, slot_of, k, M, det_label, min_birth_age, max_inactive_age, step, reset=None):
    """Kernel 1, per stream: -> staging rows per stream [(track_id, src_trk, src_det, keep, state, birth_age, inactive_age, label)], took-part
    flags; updates next_track_id and status of `st` in place.  slot_of[s]: the stream's slot, -1 no part; reset: a stream to forget;
    det_label: [L * k]."""
    S = len(slot_of)
    stage, part = [], []
    for s in range(S):
        t0, T = int(st["trk_off"][s]), int(st["trk_off"][s + 1] - st["trk_off"][s])
        slot = slot_of[s]
        rows, took, code = [], 0, 0
        if s == reset:
            st["next_track_id"][s] = 0
        else:
            if slot >= 0:
                code = int(assoc[s]["status"]) & 0xffff
            if slot < 0 or code:
                rows = [(int(st["track_id"][t0 + r]), t0 + r, -1, 0, int(st["state"][t0 + r]), int(st["birth_age"][t0 + r]),
                         int(st["inactive_age"][t0 + r]), int(st["label"][t0 + r])) for r in range(T)]
            else:
                a = assoc[s]
                det_of, keep = [-1] * T, [0] * T
                for d, t in a["matches"]:            # the quirk: position d of the unfiltered arrays
                    det_of[t] = d
                for d, t in a.get("low_matches") or ():
                    det_of[t], keep[t] = d, 1
                for r in range(T):
                    state, birth, inact = int(st["state"][t0 + r]), int(st["birth_age"][t0 + r]), int(st["inactive_age"][t0 + r])
                    if det_of[r] >= 0:
                        if state == UNCONFIRMED:
                            birth += 1
                            if birth >= min_birth_age:
                                state = ACTIVE
                        elif state == INACTIVE:
                            state, inact = ACTIVE, 0
                    elif state == UNCONFIRMED:
                        state = TO_DELETE
                    elif state == ACTIVE:
                        state, inact = INACTIVE, 0
                    elif state == INACTIVE:
                        inact += 1
                        if inact >= max_inactive_age:
                            state = TO_DELETE
                    if state != TO_DELETE:
                        rows.append((int(st["track_id"][t0 + r]), t0 + r, slot * k + det_of[r] if det_of[r] >= 0 else -1,
                                     keep[r] if det_of[r] >= 0 else 0, state, birth, inact, int(st["label"][t0 + r])))
                room = M - len(rows)
                born = list(a["unmatched_dets"])[:max(room, 0)]
                if len(a["unmatched_dets"]) > room:
                    code = OVERFLOW
                nid = int(st["next_track_id"][s])
                for q, row in enumerate(born):
                    src = int(a["det_index"][row])
                    rows.append((nid + q, -1, slot * k + src, 0, UNCONFIRMED, 0, 0, int(det_label[slot * k + src])))
                st["next_track_id"][s] = nid + len(born)
                took = 1
        if code:
            have = int(st["status"][s, 0])
            if have == 0:
                st["status"][s, 1] = step
            st["status"][s, 0] = have | (code & OVERFLOW) | ((code & 0xffff) if (have & 0xffff) == 0 else 0)
        stage.append(rows)
        part.append(took)
    return stage, part


def pack(st, stage, part, M):
    """Kernel 2: -> (new state without its boxes, lists dict(src_trk, src_det, keep_emb, flags, eligible) over the capacity)."""
    S = len(stage)
    C = S * M
    new = new_state(S, M)
    new["next_track_id"], new["status"] = st["next_track_id"], st["status"]
    new["trk_off"][1:] = np.cumsum([len(r) for r in stage])
    lists = dict(src_trk=np.arange(C, dtype=np.int32), src_det=np.full(C, -1, np.int32), keep_emb=np.zeros(C, np.uint8), flags=np.zeros(C, np.int32),
                 eligible=np.zeros(C, np.uint8))
    r = 0
    for s in range(S):
        for tid, src_trk, src_det, keep, state, birth, inact, label in stage[s]:
            new["track_id"][r], new["state"][r], new["birth_age"][r], new["inactive_age"][r], new["label"][r] = tid, state, birth, inact, label
            lists["src_trk"][r], lists["src_det"][r], lists["keep_emb"][r], lists["flags"][r] = src_trk, src_det, keep, part[s]
            lists["eligible"][r] = state == ACTIVE
            r += 1
    return new, lists


def emit(st, new, lists, live, M, det_box, kalman_box=None):
    """Kernel 3: fills new["box"]; -> the step's outputs (bboxes [L, M, 4] float32 | float64 with kalman_box, track_ids, labels int64 [L, M],
    count int32 [L]).  det_box: [L * k, 4] float32; kalman_box: the filter's out_box [C, 4] float64 or None."""
    rows = int(new["trk_off"][-1])
    for r in range(rows):
        d, t = int(lists["src_det"][r]), int(lists["src_trk"][r])
        new["box"][r] = (kalman_box[r] if kalman_box is not None else det_box[d].astype(np.float64)) if d >= 0 else st["box"][t]
    L = len(live)
    out = dict(bboxes=np.zeros((L, M, 4), np.float32 if kalman_box is None else np.float64), track_ids=np.zeros((L, M), np.int64),
               labels=np.zeros((L, M), np.int64), count=np.zeros(L, np.int32))
    for i, s in enumerate(live):
        act = [r for r in range(int(new["trk_off"][s]), int(new["trk_off"][s + 1])) if new["state"][r] == ACTIVE]
        out["count"][i] = len(act)
        out["bboxes"][i, :len(act)] = new["box"][act]
        out["track_ids"][i, :len(act)] = new["track_id"][act]
        out["labels"][i, :len(act)] = new["label"][act]
    return out


def step(st, assoc, live, k, M, det_box, det_label, min_birth_age, max_inactive_age, step_no, kalman_box=None, reset=None):
    """One step of the three kernels: (new state, lists, outputs).  live: the participating streams in slot order; reset: a stream to forget."""
    S = len(st["next_track_id"])
    slot_of = [-1] * S
    for i, s in enumerate(live):
        slot_of[s] = i
    stage, part = lifecycle(st, assoc, slot_of, k, M, det_label, min_birth_age, max_inactive_age, step_no, reset)
    new, lists = pack(st, stage, part, M)
    return new, lists, emit(st, new, lists, live, M, det_box, kalman_box)
