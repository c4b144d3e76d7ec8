"""A serial model of k_deflate_segments' parse (patolette_amd/csrc/deflate.hip): which tokens the coder writes.

Plain Python, one position after the other, from the rules as DESIGN.md and the kernel's comments state them; no lanes, no masks.
`model_tokens(filtered, row_bytes, segment)` returns, per segment of one frame's filtered stream, the token list (an int for a
literal, a (length, distance) pair for a match -- tests/deflate_trace.py's form, without the end of block) and a trace of the rules
that fired.  `mutation` names ONE rule to get wrong (MUTATIONS): tests/test_deflate_model.py proves with them that the inputs of
tests/test_gpu_png_tokens.py tell the true rules from their neighbours.

The rules:
  * a segment is parsed in steps of 64 positions counted from its start; a step that an earlier match covers whole is skipped: none
    of its positions enter the hash table, the waiting counter does not move, the previous step's token count stays;
  * a position with at least three bytes left in the segment has a key, its three bytes, in slot (key * 2654435761 mod 2^32) >> 20 of
    a table that keeps the HIGHEST position entered; a step's lookups all see the table as it was before the step, and after them
    every keyed position of the step enters it, the covered ones in front of a partly covered step too;
  * a match at position i (of the segment that starts at byte q0 of the frame) may start up to reach = min(q0 + i, 32768) bytes back
    and is at most min(258, len - i) bytes long; the distances are tried in the order 1, 2, 4, 8, R-1, R, R+1, 2R, 4R, 8R (R the row's
    bytes), the four remembered ones, the hashed one, and only a strictly longer match replaces the best: the first in this order
    among equals; a best below three bytes, or of three bytes further back than 4096, is dropped;
  * the walk takes the match at p unless p + 1 lies in the same step and has a longer one (then p is a literal), and jumps;
  * when the step before left more than two tokens (before the first step: 64) and no wait is pending, the step explores first: at its
    first free position every distance up to the reach is tried, the longest wins, then the nearest; eight bytes and more move the
    distance to the front of the remembered four (found at place 0, 1, 2: the ones before it move down; else the last drops out);
    less counts as a failure, as does an anchor with fewer than four bytes left, and after the n-th failure in a row the next
    explorations wait 1, 3, 7, 15, 15, ... steps (a wait moves only in a step that would have explored)."""
STEP, MIN_MATCH, MAX_MATCH, WINDOW, FAR = 64, 3, 258, 32768, 4096
EXPLORE_TOKENS, EXPLORE_MIN = 2, 8
FIXED = ("1", "2", "4", "8", "R-1", "R", "R+1", "2R", "4R", "8R")
NAMES = FIXED + ("rep0", "rep1", "rep2", "rep3", "hash")

MUTATIONS = {
    **{"no_" + name: "the candidate %s is never tried" % name for name in FIXED},
    "tie_nearest": "among equal lengths the nearer distance wins",
    "hash_after_insert": "the table is read after the step's own positions entered it",
    "hash_first_wins": "a slot keeps the first position entered, not the last",
    "hash_skipped_steps": "the positions of a wholly skipped step enter the table",
    "lazy_off": "no lazy evaluation",
    "lazy_across_steps": "lazy evaluation looks at p + 1 in the next step too",
    "far_4095": "a three-byte match is dropped beyond 4095",
    "reach_in_segment": "reach = i: no match starts before the segment",
    "reach_32767": "the window ends a byte early",
    "max_257": "a match is at most 257 bytes",
    "explore_tokens_1": "an exploration runs after more than 1 token",
    "explore_tokens_3": "an exploration runs after more than 3 tokens",
    "explore_min_7": "7 bytes suffice for an exploration to succeed",
    "wait_1_2_4_8": "the waits are 1, 2, 4, 8, 8, ...",
    "rotate_push_only": "a distance found at place 1 or 2 is pushed in front like a new one",
}


def match_length(data, a, c, maxlen):
    """bytes from a and from c (c < a; they may overlap) that agree, at most maxlen"""
    k = 0
    while k + 16 <= maxlen and data[a + k:a + k + 16] == data[c + k:c + k + 16]:
        k += 16
    while k < maxlen and data[a + k] == data[c + k]:
        k += 1
    return k


def slot_of(b0, b1, b2):
    return (((b0 | b1 << 8 | b2 << 16) * 2654435761) & 0xFFFFFFFF) >> 20


def new_trace():
    """What fired in a segment.  Counts unless said otherwise; the entries below `explore_log` are taken at the positions the walk
    visits (a token's start, or the p + 1 a lazy step looks at)."""
    return dict(
        longest_match=0, longest_distance=0,
        before_segment=0,                                               # matches whose source starts before the segment
        lazy=0, far_dropped=0, skipped_steps=0,
        explorations=0, explored=0,                                     # run, and succeeded
        rotation=dict(rep0=0, rep1=0, rep2=0, new=0),
        waits_served=[], longest_wait=0,                                # every wait that ran out, in order
        hash_won=0,
        winners=dict.fromkeys(NAMES, 0),                                # the matches taken, by the candidate that gave them
        sole=dict.fromkeys(NAMES, 0),                                   # ... where no other candidate, by value or length, could have
        tie_far=0,                                                      # matches taken over an equally long one at a NEARER candidate distance
        success_after_failures=0,                                       # the most failures in a row that a success ended
        short_anchor=0,                                                 # explorations whose anchor had 4 .. 7 bytes left
        explore_log=[],                                                 # (anchor, length, distance, failures before) of every exploration
        distance_32768=0, match_258_then_match=0, ends_at_last_byte=0, three_at_4096=0,
        no_look_across_steps=0,                                         # matches at a step's last position with a longer one right behind it
        slot_collisions=0,                                              # lookups that found another key in their slot
        unseen_same_step=0,                                             # lookups whose key occurs earlier in their own step
        key_in_skipped_step=0)                                          # lookups whose key last occurred in a wholly skipped step


def model_tokens(filtered, row_bytes, segment, mutation=None):
    """([tokens of segment 0, ...], [trace of segment 0, ...]) of one frame's filtered stream."""
    assert mutation is None or mutation in MUTATIONS, mutation
    data, R, total = bytes(filtered), int(row_bytes), len(filtered)
    assert total >= 1 and R >= 2 and 1 <= segment <= WINDOW
    m = mutation
    max_match = 257 if m == "max_257" else MAX_MATCH
    window = 32767 if m == "reach_32767" else WINDOW
    far = 4095 if m == "far_4095" else FAR
    explore_tokens = 1 if m == "explore_tokens_1" else 3 if m == "explore_tokens_3" else EXPLORE_TOKENS
    explore_min = 7 if m == "explore_min_7" else EXPLORE_MIN
    fixed = [1, 2, 4, 8, R - 1, R, R + 1, 2 * R, 4 * R, 8 * R]
    if m is not None and m.startswith("no_"):
        fixed[FIXED.index(m[3:])] = 0
    out_tokens, out_traces = [], []

    for q0 in range(0, total, segment):
        n = min(segment, total - q0)
        tokens, tr = [], new_trace()
        table = {}                                                      # slot -> position + 1
        last_step, skipped = {}, set()                                  # (trace) key -> the last step that held it; the skipped steps
        reps = [0, 0, 0, 0]
        prev_tokens, wait, wait_set, fails, skip = STEP, 0, 0, 0, 0

        def limits(i):
            reach = min(i if m == "reach_in_segment" else q0 + i, window)
            return min(max_match, n - i), reach

        def enter(b0, cnt):
            for i in range(b0, b0 + cnt):
                if n - i >= MIN_MATCH:
                    s = slot_of(data[q0 + i], data[q0 + i + 1], data[q0 + i + 2])
                    if m != "hash_first_wins" or s not in table:
                        table[s] = i + 1

        def best_at(i, count=True):
            """(length, distance, index of the winning candidate, the candidates) at position i"""
            maxlen, reach = limits(i)
            if maxlen < MIN_MATCH:
                return 0, 0, -1, None
            a = q0 + i
            key = data[a:a + 3]
            seen = table.get(slot_of(*key), 0)
            if count and m is None:
                b0 = i - i % STEP
                tr["slot_collisions"] += bool(seen) and data[q0 + seen - 1:q0 + seen + 2] != key
                tr["unseen_same_step"] += data.find(key, q0 + b0, a + 2) >= 0
                tr["key_in_skipped_step"] += last_step.get(key) in skipped
            cands = fixed + reps + [i + 1 - seen if seen else 0]
            best, dist, who = 0, 0, -1
            for j, d in enumerate(cands):
                if d <= 0 or d > reach or best >= maxlen:
                    continue
                l = match_length(data, a, a - d, maxlen)
                if l > best or (m == "tie_nearest" and l == best and l > 0 and d < dist):
                    best, dist, who = l, d, j
            if best == MIN_MATCH and dist > far:
                tr["far_dropped"] += count
                best = 0
            if best < MIN_MATCH:
                return 0, 0, -1, None
            return best, dist, who, cands

        for b0 in range(0, n, STEP):
            cnt = min(STEP, n - b0)
            if skip >= cnt:
                skip -= cnt
                tr["skipped_steps"] += 1
                skipped.add(b0 // STEP)
                if m == "hash_skipped_steps":
                    enter(b0, cnt)
                if m is None:
                    for i in range(b0, min(b0 + cnt, n - 2)):
                        last_step[data[q0 + i:q0 + i + 3]] = b0 // STEP
                continue
            # ---- the exploration
            if prev_tokens > explore_tokens:
                if wait:
                    wait -= 1
                    if wait == 0:
                        tr["waits_served"].append(wait_set)
                        tr["longest_wait"] = max(tr["longest_wait"], wait_set)
                else:
                    ai = b0 + skip
                    amax, areach = limits(ai)
                    a = q0 + ai
                    wl = wd = 0
                    tr["explorations"] += 1
                    if amax >= 4:
                        tr["short_anchor"] += amax < 8
                        prefix, c = data[a:a + 4], a
                        while wl < amax:                                # every earlier place with the anchor's four bytes, the nearest first
                            c = data.rfind(prefix, a - areach, c + 3)
                            if c < 0:
                                break
                            l = match_length(data, a, c, amax)
                            if l > wl:
                                wl, wd = l, a - c
                    tr["explore_log"].append((ai, wl, wd, fails))
                    if wl >= explore_min:
                        tr["explored"] += 1
                        tr["success_after_failures"] = max(tr["success_after_failures"], fails)
                        fails = 0
                        if wd == reps[0]:
                            tr["rotation"]["rep0"] += 1
                        elif wd == reps[1] and m != "rotate_push_only":
                            tr["rotation"]["rep1"] += 1
                            reps = [wd, reps[0], reps[2], reps[3]]
                        elif wd == reps[2] and m != "rotate_push_only":
                            tr["rotation"]["rep2"] += 1
                            reps = [wd, reps[0], reps[1], reps[3]]
                        else:
                            tr["rotation"]["new"] += 1
                            reps = [wd, reps[0], reps[1], reps[2]]
                    else:
                        fails += 1
                        wait = min(1 << (fails - 1), 8) if m == "wait_1_2_4_8" else min(1 << min(fails, 5), 16) - 1
                        wait_set = wait
            # ---- every visited position's best match, against the table as the step found it
            if m == "hash_after_insert":
                enter(b0, cnt)
            found = {}

            def best(p):
                if p not in found:
                    found[p] = best_at(b0 + p)
                return found[p]

            # ---- the walk
            p, step_tokens = skip, 0
            while p < cnt:
                L, D, who, cands = best(p)
                if L and m != "lazy_off":
                    if p + 1 < cnt:
                        if best(p + 1)[0] > L:
                            L = 0
                            tr["lazy"] += 1
                    elif b0 + p + 1 < n and m in (None, "lazy_across_steps") and best_at(b0 + p + 1, False)[0] > L:
                        if m is None:
                            tr["no_look_across_steps"] += 1             # p + 1 is the next step's: the walk does not look there
                        else:
                            L = 0
                i = b0 + p
                if L:
                    note_match(tr, data, q0, n, i, L, D, who, cands, tokens, limits(i), m)
                    tokens.append((L, D))
                    p += L
                else:
                    tokens.append(data[q0 + i])
                    p += 1
                step_tokens += 1
            skip = p - cnt
            if m is None:
                for i in range(b0, min(b0 + cnt, n - 2)):
                    last_step[data[q0 + i:q0 + i + 3]] = b0 // STEP
            if m != "hash_after_insert":
                enter(b0, cnt)
            prev_tokens = step_tokens
        out_tokens.append(tokens)
        out_traces.append(tr)
    return out_tokens, out_traces


def note_match(tr, data, q0, n, i, L, D, who, cands, tokens, lim, m):
    """the trace's entries for the match (L, D) taken at position i"""
    tr["longest_match"] = max(tr["longest_match"], L)
    tr["longest_distance"] = max(tr["longest_distance"], D)
    tr["before_segment"] += D > i
    tr["distance_32768"] += D == WINDOW
    tr["ends_at_last_byte"] += i + L == n
    tr["three_at_4096"] += L == 3 and D == FAR
    tr["match_258_then_match"] += bool(tokens) and isinstance(tokens[-1], tuple) and tokens[-1][0] == MAX_MATCH
    tr["winners"][NAMES[who]] += 1
    tr["hash_won"] += NAMES[who] == "hash"
    if m is not None:
        return
    maxlen, reach = lim
    a = q0 + i
    lens = [match_length(data, a, a - d, maxlen) if 0 < d <= reach else 0 for d in cands]
    if all(lens[j] < L and cands[j] != D for j in range(len(cands)) if j != who):
        tr["sole"][NAMES[who]] += 1
    if any(lens[j] == L and 0 < cands[j] < D for j in range(len(cands))):
        tr["tie_far"] += 1
