#!/usr/bin/env python
"""The seeded rejection search behind tests/overlap_inputs.py's cases (CPU only).

For every link and both obstacle kinds it makes the draws of overlap_inputs.assemble, classifies each pair, keeps the admitted ones
(the pair in a class, every other link box clear of the grown obstacle; q is drawn inside the joint limits) and chooses the cases of the
table; for the self pairs it classifies every masked pair of the drawn configurations.  It writes

    tests/overlap_cases.json        class -> (seed, draw index, link or pair): what overlap_inputs.build turns into a case
    profiles/overlap_census.json    per class and link: draws made, pairs found, the chosen cases' slack; the caps, and what was not found

Among the admitted pairs of a (class, link) cell the one with the largest slack (distance inside its class beyond M) is taken; a CAP case of
a face whose axes the rule exchanges must also change its verdict under overlap_inputs.cylinder_rule(half_swap=True).

    python scripts/overlap_census.py [--box-draws 60000] [--cyl-draws 60000] [--self-draws 20000]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from edmp_amd import franka  # noqa: E402
from oracle import success_oracle as SO  # noqa: E402
from tests import overlap_inputs as OI  # noqa: E402

CHUNK = 20000
KEEP = 8  # candidates kept per (class, link) cell, by slack
SCALE = {8: 0.3}  # the finger box is a few centimetres: its obstacles are scaled to it
BOX_SEED, CYL_SEED, SELF_SEED = 100, 200, 300


def search(link, kind, seed, draws, n_codes):
    """-> found (n_codes,) counts of admitted pairs, in_class (n_codes,) counts before the clearance of the other links, best {code: [(slack, index)] by falling slack}"""
    scale = SCALE.get(link, 1.0)
    found, in_class, best = np.zeros(n_codes, dtype=int), np.zeros(n_codes, dtype=int), {}
    for start in range(0, draws, CHUNK):
        idx = np.arange(start, min(start + CHUNK, draws))
        P = np.stack([OI.params(seed, i) for i in idx])
        Q, OC = OI.assemble(P, link, kind, scale)
        code, slack, clear = OI.classify_link_cases(Q, OC, link, kind)
        for c in np.unique(code[code >= 0]):
            sel = code == c
            in_class[c] += int(sel.sum())
            sel &= clear
            found[c] += int(sel.sum())
            for k in np.nonzero(sel)[0][np.argsort(-slack[sel])[:KEEP]]:
                best.setdefault(int(c), []).append((float(slack[k]), int(idx[k])))
    return found, in_class, {c: sorted(v, reverse=True)[:KEEP] for c, v in best.items()}


def half_swap_flips(entry):
    """a CAP case of a face whose axes the rule exchanges: the rule with the exchange done by halves must give another verdict"""
    case = OI.build(entry)
    Rl, cl = SO.link_box_poses(case["q"])[case["link"]]
    Ro, co, (rad, H) = OI.obstacle_shape(case["oc"], 1)
    he = OI.HE[case["link"]]
    return OI.cylinder_rule(Rl, cl, he, Ro, co, rad, H) != OI.cylinder_rule(Rl, cl, he, Ro, co, rad, H, half_swap=True)


def first_admitted(name, link, candidates):
    """the cell's candidate of the largest slack; for a CAP class of an exchanged face, the first whose verdict the half exchange changes"""
    for slack, index in candidates:
        entry = dict(cls=name, kind=1, link=link, seed=CYL_SEED + link, index=index, scale=SCALE.get(link, 1.0), slack=slack)
        if not (name.startswith("CAP") and name.endswith("_1")) or half_swap_flips(entry):
            return entry
    return None


def caps_unmet(census):
    """the caps of the table that the census does not meet, as sentences (the host test checks them again on the built cases)"""
    caps, out = census["caps"], list(census["not_found"])
    if min(caps["box_cases_per_link"]) < 3:
        out.append("a link with fewer than 3 box cases")
    if len(caps["cap_classes_present"]) < 24 or not set(range(8)) <= set(caps["cap_links"]):
        out.append("a CAP class or a link 0..7 without a CAP case")
    if len(caps["edge_classes_absent"]) > 2:
        out.append("more than 2 EDGE classes absent")
    if len(caps["self_pairs_used"]) < 8:
        out.append("fewer than 8 self pairs")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--box-draws", type=int, default=60000, help="per link")
    ap.add_argument("--cyl-draws", type=int, default=60000, help="per link")
    ap.add_argument("--self-draws", type=int, default=20000)
    args = ap.parse_args()
    cases, census = [], dict(margin_m=OI.M, clearance_m=OI.CLEAR, box={}, cylinder={}, self={}, not_found=[], caps={})

    # ---- boxes: every SEP_k / TIGHT_k on three links, the links dealt round
    cells = {}
    for link in range(9):
        found, in_class, best = search(link, 0, BOX_SEED + link, args.box_draws, OI.N_BOX)
        for c in range(OI.N_BOX):
            census["box"].setdefault(OI.box_name(c), {})[str(link)] = dict(draws=args.box_draws, in_class=int(in_class[c]), admitted=int(found[c]))
            if c in best:
                cells[(c, link)] = best[c]
        print(f"[census] boxes, link {link}: {int((found > 0).sum())}/30 classes", flush=True)
    per_link = np.zeros(9, dtype=int)
    for c in range(OI.N_BOX):
        order = [(c + 3 * t) % 9 for t in range(3)] + [l for l in range(9)]
        chosen = []
        for link in order:
            if link not in chosen and (c, link) in cells and len(chosen) < 3:
                chosen.append(link)
        for link in chosen:
            slack, index = cells[(c, link)][0]
            cases.append(dict(cls=OI.box_name(c), kind=0, link=link, seed=BOX_SEED + link, index=index, scale=SCALE.get(link, 1.0), slack=slack))
            per_link[link] += 1
        if len(chosen) < 3:
            census["not_found"].append(f"{OI.box_name(c)}: on {len(chosen)} links only")
    census["caps"]["box_classes_on_3_links"] = not any(s.startswith(("SEP", "TIGHT")) for s in census["not_found"])
    census["caps"]["box_cases_per_link"] = per_link.tolist()

    # ---- cylinders
    cells, totals = {}, np.zeros(OI.N_CYL, dtype=int)
    for link in range(9):
        found, in_class, best = search(link, 1, CYL_SEED + link, args.cyl_draws, OI.N_CYL)
        totals += found
        for c in range(OI.N_CYL):
            census["cylinder"].setdefault(OI.cylinder_name(c), {})[str(link)] = dict(draws=args.cyl_draws, in_class=int(in_class[c]), admitted=int(found[c]))
            if c in best:
                cells[(c, link)] = best[c]
        print(f"[census] cylinders, link {link}: {int((found > 0).sum())}/38 classes", flush=True)
    cap_links = set()
    for c in range(OI.N_CYL):
        name = OI.cylinder_name(c)
        want = 3 if c in (0, OI.CODE_MISS) else 2
        links = sorted((l for l in range(9) if (c, l) in cells), key=lambda l: ((l - c) % 9))
        chosen = []
        for link in links:
            if len(chosen) == want:
                break
            entry = first_admitted(name, link, cells[(c, link)])
            if entry is None:
                continue
            chosen.append(link)
            cases.append(entry)
            if name.startswith("CAP"):
                cap_links.add(link)
        if len(chosen) < (3 if c in (0, OI.CODE_MISS) else 1):
            census["not_found"].append(f"{name}: {len(chosen)} cases after {9 * args.cyl_draws} draws")
    # a CAP case on every link that has one and is not covered yet
    for link in range(9):
        if link in cap_links:
            continue
        for c in range(13, OI.CODE_MISS):
            if (c, link) in cells:
                entry = first_admitted(OI.cylinder_name(c), link, cells[(c, link)])
                if entry is None:
                    continue
                cases.append(entry)
                cap_links.add(link)
                break
    census["caps"]["cap_links"] = sorted(cap_links)
    census["caps"]["cap_classes_present"] = sorted({c["cls"] for c in cases if c["cls"].startswith("CAP")})
    census["caps"]["edge_classes_absent"] = [OI.cylinder_name(c) for c in range(1, 13) if not any(k["cls"] == OI.cylinder_name(c) for k in cases)]
    for face, sign in ((0, 1), (1, -1)):
        for hit in (1, 0):
            cases.append(dict(cls="ZEROS_HIT" if hit else "ZEROS_MISS", zeros=[face, sign, hit]))

    # ---- self pairs: every SEP_k / TIGHT_k once, the pairs dealt round
    pairs = [(a, b) for a in range(9) for b in range(a + 1, 9) if franka.self_collision_pairs()[a, b]]
    Q = np.stack([OI.params(SELF_SEED, i)[:7] for i in range(args.self_draws)])
    cells = {}
    for p, (a, b) in enumerate(pairs):
        code, slack = OI.classify_self_cases(Q, a, b)
        for c in np.unique(code[code >= 0]):
            sel = code == c
            k = int(np.argmax(np.where(sel, slack, -np.inf)))
            cells[(int(c), p)] = (float(slack[k]), k)
            census["self"].setdefault(OI.box_name(int(c)), {})[f"{a}-{b}"] = dict(draws=args.self_draws, in_class=int(sel.sum()))
    used = set()
    for c in range(OI.N_BOX):
        order = sorted((p for p in range(len(pairs)) if (c, p) in cells), key=lambda p: ((p - 7 * c) % len(pairs)))
        if not order:
            census["not_found"].append(f"self {OI.box_name(c)}: in none of {args.self_draws} configurations")
            continue
        p = order[0]
        slack, index = cells[(c, p)]
        cases.append(dict(cls=OI.box_name(c), pair=list(pairs[p]), seed=SELF_SEED, index=index, slack=slack))
        used.add(p)
    census["caps"]["self_pairs_used"] = [list(pairs[p]) for p in sorted(used)]
    census["cases"] = len(cases)
    census["chosen"] = [{k: v for k, v in c.items()} for c in cases]
    with open(OI.TABLE, "w") as f:
        json.dump(dict(margin_m=OI.M, cases=[{k: v for k, v in c.items() if k != "slack"} for c in cases]), f, indent=0)
    with open(os.path.join(ROOT, "profiles", "overlap_census.json"), "w") as f:
        json.dump(census, f, indent=1)
    unmet = caps_unmet(census)
    if unmet:
        sys.exit(f"[census] caps not met: {unmet}")
    print(f"[census] {len(cases)} cases; not found: {census['not_found']}; edge classes absent: {census['caps']['edge_classes_absent']}")


if __name__ == "__main__":
    main()
