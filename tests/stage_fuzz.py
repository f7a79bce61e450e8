"""A deterministic generator of Stage sets and objects for an invented unstructured kind
(`example.com/v1 Gadget`), and the oracle run the fuzz tests share (tests/test_stage_fuzz.py on
the CPU, tests/test_gpu_stage_fuzz.py on the engine).

`make_case(seed, **params) -> (stage_docs, objs)` draws everything from `random.Random(seed)`: the
v1alpha1 Stage documents a user could write (selectors over labels, annotations, two status
fields, the deletion timestamp and the finalizer set; weight / delay / jitter getters with and
without `*From` expressions; static status templates, delete, finalizer edits) and the objects
they run on.  Templates carry no `{{` actions, so the oracle (`oracle/next_ref.render_status`)
applies them as plain YAML.  The generator counts the feature bits the set will need (one per
distinct Exists/DoesNotExist key, one per In/NotIn literal, one per finalizer value + 1, one per
possibly idempotent patch) and stays within `max_bits`.

Two modes: `loops=False` makes every patch falsify a requirement of its own stage (no "patch
already applied" bits arise, the native encoder accepts the program); `loops=True` lets idempotent
patches keep matching (applied bits, re-match suppression, state-dependent deltas)."""
from __future__ import annotations

import functools
import json
import random
from typing import Dict, List, Optional, Tuple

API_GROUP, KIND = "example.com/v1", "Gadget"
NOW0 = 1_700_000_000 * 10**9  # 2023-11-14T22:13:20Z
INT64_MAX = (1 << 63) - 1

PHASE, NUM, DELETION, FINS = ".status.phase", ".status.n", ".metadata.deletionTimestamp", ".metadata.finalizers.[]"
PHASES = ["Pending", "Running", "Done", "Failed", "Stuck", "Idle"]
NUMS = [0, 1, 2, 3]
LABELS = {"tier": ["gold", "silver", "bronze"], "zone": ["a", "b", "c"]}
ANNOTATIONS = {"mode": ["fast", "slow", "off"]}
FIN_VALUES = ["example.com/fa", "example.com/fb"]
FIN_UNKNOWN = "example.com/zz"  # on objects only: the finalizer set's "other" bit
W_ANN, D_ANN, J_ANN = "gadget.example.com/weight", "gadget.example.com/delay", "gadget.example.com/jitter"
W_VALUES = ["3", "1", "0", "-2", "bad", "0x10", " 4", str(INT64_MAX)]
D_VALUES = ["1s", "1500ms", "2m", "-5s", "bad", "2023-11-14T22:13:00Z", "2023-11-14T22:13:25Z",
            "2023-11-14T22:14:10Z"]  # Go durations, RFC3339 before the clock and after it
J_VALUES = ["2s", "10s", "0s", "bad", "90s"]
DEL_VALUES = ["2023-11-14T22:13:10Z", "2023-11-14T22:13:23Z", "2023-11-14T22:14:10Z"]
WEIGHTS = [None, 0, 1, 2, 100, -1, 1 << 40]
DURATIONS_MS = [None, 0, 1, 500, 60000]

# the clock of every run: 1 s steps, a 35 s jump (the fused record's epoch moves), one step
# backwards, and a second jump past the 60 s delays
CLOCK_S = [0, 1, 2, 3, 38, 39, 37, 40, 41, 75, 76, 77]
NOWS = [NOW0 + s * 10**9 for s in CLOCK_S]
RUN_SEED = 0x46555A5A


def label_key(k: str) -> str:
    return ".metadata.labels[%s]" % json.dumps(k)


def annotation_key(k: str) -> str:
    return ".metadata.annotations[%s]" % json.dumps(k)


class _Bits:
    """The feature bits a Stage set costs, counted as the stage compiler assigns them."""

    def __init__(self, limit: int):
        self.limit = limit
        self.atoms = set()

    def cost(self, atoms) -> int:
        return len(set(atoms) - self.atoms)

    def fits(self, atoms) -> bool:
        return len(self.atoms) + self.cost(atoms) <= self.limit

    def take(self, atoms):
        self.atoms |= set(atoms)
        assert len(self.atoms) <= self.limit

    @property
    def used(self) -> int:
        return len(self.atoms)


def _req_atoms(r: dict):
    if r["key"] == FINS:
        a = [("fin", "other")]
        return a + [("fin", v) for v in r.get("values", [])]
    if r["operator"] in ("Exists", "DoesNotExist"):
        return [("present", r["key"])]
    return [("lit", r["key"], v) for v in r["values"]]


def _req(key, op, values=None):
    r = {"key": key, "operator": op}
    if values is not None:
        r["values"] = [str(v) for v in values]
    return r


class _Gen:
    def __init__(self, seed: int, p: dict):
        self.rng = random.Random(seed)
        self.p = p
        self.keys = list(p["keys"])
        self.phases = PHASES[:p["n_phases"]]
        self.bits = _Bits(p["max_bits"])

    # -- selectors
    def _values(self, key):
        if key == PHASE:
            return self.phases
        if key == NUM:
            return NUMS
        if key == FINS:
            return FIN_VALUES
        for table, mk in ((LABELS, label_key), (ANNOTATIONS, annotation_key)):
            for k, vs in table.items():
                if mk(k) == key:
                    return vs
        raise KeyError(key)

    def _key_pool(self):
        pool = []
        if "phase" in self.keys:
            pool += [PHASE] * 3
        if "n" in self.keys:
            pool += [NUM] * 2
        if "labels" in self.keys:
            pool += [label_key(k) for k in LABELS]
        if "annotations" in self.keys:
            pool += [annotation_key(k) for k in ANNOTATIONS]
        if "deletion" in self.keys:
            pool += [DELETION]
        if "finalizers" in self.keys:
            pool += [FINS]
        return pool

    def requirement(self, key=None, multi_in=False):
        """One matchExpressions entry within the bit budget (a few draws, then one that costs
        nothing new)."""
        rng = self.rng
        for _ in range(12):
            k = key or rng.choice(self._key_pool())
            if k == DELETION:
                r = _req(k, rng.choice(["Exists", "DoesNotExist"]))
            else:
                op = "In" if multi_in else rng.choice(["In", "In", "NotIn", "Exists", "DoesNotExist"])
                if op in ("In", "NotIn"):
                    vs = self._values(k)
                    n = rng.randint(2, min(3, len(vs))) if multi_in else rng.choice([1, 1, 2, 3])
                    r = _req(k, op, rng.sample(vs, min(n, len(vs))))
                else:
                    r = _req(k, op)
            if self.bits.fits(_req_atoms(r)):
                self.bits.take(_req_atoms(r))
                return r
        return self.free_requirement(multi_in)

    def free_requirement(self, multi_in=False):
        """A requirement over bits the set already has."""
        rng = self.rng
        lits: Dict[str, List[str]] = {}
        for a in sorted(self.bits.atoms):
            if a[0] == "lit":
                lits.setdefault(a[1], []).append(a[2])
        if multi_in:
            ks = sorted(k for k, v in lits.items() if len(v) >= 2)
            if ks:
                k = rng.choice(ks)
                return _req(k, "In", rng.sample(lits[k], rng.randint(2, min(3, len(lits[k])))))
        if lits:
            k = rng.choice(sorted(lits))
            return _req(k, rng.choice(["In", "NotIn"]), [rng.choice(lits[k])])
        pres = sorted(a[1] for a in self.bits.atoms if a[0] == "present")
        if pres:
            return _req(rng.choice(pres), rng.choice(["Exists", "DoesNotExist"]))
        raise AssertionError("no feature bit to reuse: max_bits too small for the first stage")

    def same_key_pair(self, contradictory: bool):
        """Two requirements on one key: compatible, or excluding each other."""
        rng = self.rng
        k = rng.choice([x for x in self._key_pool() if x != FINS] or [PHASE])
        if contradictory:
            if k == DELETION or rng.random() < 0.5:
                pair = [_req(k, "DoesNotExist"), _req(k, "Exists")]
            else:
                v = rng.choice(self._values(k))
                pair = [_req(k, "In", [v]), _req(k, "NotIn", [v])]
            if rng.random() < 0.5:
                pair.reverse()
        elif k == DELETION:
            pair = [_req(k, "Exists"), _req(k, "Exists")]
        else:
            vs = self._values(k)
            v = rng.choice(vs)
            other = rng.choice([x for x in vs if x != v])
            pair = rng.choice([[_req(k, "Exists"), _req(k, "In", [v])],
                               [_req(k, "In", [v]), _req(k, "NotIn", [other])],
                               [_req(k, "NotIn", [v]), _req(k, "NotIn", [other])]])
        atoms = [a for r in pair for a in _req_atoms(r)]
        if not self.bits.fits(atoms):
            return [self.free_requirement()]
        self.bits.take(atoms)
        return pair

    # -- next
    def guard_and_patch(self):
        """loops=False: a requirement and a status patch that falsifies it."""
        rng = self.rng
        if self.p["chain"]:  # stage j alone matches phase j: no state has two candidates
            g = self.chain_guard()
            return g, {"phase": rng.choice([v for v in self.phases if v != g["values"][0]] + [None])}
        field = PHASE if ("phase" in self.keys and ("n" not in self.keys or rng.random() < 0.7)) else NUM
        vs = self._values(field)
        name = "phase" if field == PHASE else "n"
        for _ in range(12):
            # a JSON number is a float64 to hasValue and equals no literal: In / NotIn cannot guard on n
            form = rng.choice(["In", "In", "In", "NotIn", "DoesNotExist", "Exists"] if field == PHASE else
                              ["DoesNotExist", "Exists"])
            if form == "In":
                s = rng.sample(vs, rng.choice([1, 1, 2]))
                rest = [v for v in vs if v not in s]
                g, patch = _req(field, "In", s), {name: rng.choice(rest + [None])}
            elif form == "NotIn":
                s = rng.sample(vs, rng.choice([1, 2]))
                g, patch = _req(field, "NotIn", s), {name: rng.choice(s)}
            elif form == "DoesNotExist":
                g, patch = _req(field, "DoesNotExist"), {name: rng.choice(vs)}
            else:
                g, patch = _req(field, "Exists"), {name: None}
            if self.bits.fits(_req_atoms(g)):
                self.bits.take(_req_atoms(g))
                return g, patch
        # no room for a new bit: guard on a status literal the set already has
        lit = sorted(a for a in self.bits.atoms if a[0] == "lit" and a[1] == PHASE)
        assert lit, "max_bits too small: no status literal to guard a patch with"
        _, key, v = rng.choice(lit)
        other = rng.choice([x for x in self._values(key) if str(x) != v])
        return _req(key, "In", [v]), {"phase": other}

    def chain_guard(self):
        g = _req(PHASE, "In", [self.phases[self.index]])
        self.bits.take(_req_atoms(g))
        return g

    def loose_patch(self):
        """loops=True: one or two status fields set or nulled, whatever the selector asks."""
        rng = self.rng
        patch = {}
        for f in rng.sample(["phase", "n", "note"], 2 if rng.random() < self.p["p_two_fields"] else 1):
            if f == "phase":
                patch[f] = rng.choice(self.phases + [None])
            elif f == "n":
                patch[f] = rng.choice(NUMS + [None])
            else:
                patch[f] = rng.choice(["x", "y"])
        return patch

    @staticmethod
    def template(patch: dict) -> str:
        return "".join("%s: %s\n" % (k, "null" if v is None else json.dumps(v)) for k, v in patch.items())

    # -- getters
    def getters(self, spec: dict):
        rng, p = self.rng, self.p
        if p["weights"]:
            w = rng.choice(WEIGHTS if rng.random() < p["odd_weights"] else [None, 0, 1, 2, 100])
            if w is not None:
                spec["weight"] = w
            if rng.random() < p["p_from"]:
                spec["weightFrom"] = {"expressionFrom": annotation_key(W_ANN)}
        if rng.random() < p["p_delay"]:
            d = {}
            ms = rng.choice(DURATIONS_MS)
            if ms is not None:
                d["durationMilliseconds"] = ms
            if rng.random() < p["p_from"]:
                src = DELETION if rng.random() < 0.4 else annotation_key(D_ANN)
                d["durationFrom"] = {"expressionFrom": src}
            if p["jitter"] and rng.random() < 0.6:
                base = ms or 0
                d["jitterDurationMilliseconds"] = rng.choice([max(0, base - 1), base, base + 1500, base + 7000])
            if p["jitter"] and rng.random() < p["p_from"] * 0.5:
                d["jitterDurationFrom"] = {"expressionFrom": annotation_key(J_ANN)}
            spec["delay"] = d

    # -- one stage
    def stage(self, i: int, kind: str, n_any: int = 0, pair: Optional[str] = None) -> dict:
        rng, p = self.rng, self.p
        exprs, nxt = [], {}
        self.index = i
        if p["chain"] and kind != "patch":
            exprs.append(self.chain_guard())
        if kind == "patch":
            if p["loops"]:
                if rng.random() < p["p_guard"]:
                    exprs.append(self.requirement(PHASE if "phase" in self.keys else None))
                nxt["statusTemplate"] = self.template(self.loose_patch())
            else:
                g, patch = self.guard_and_patch()
                exprs.append(g)
                if rng.random() < 0.3:
                    patch["note"] = rng.choice(["x", "y"])
                nxt["statusTemplate"] = self.template(patch)
        elif kind == "delete":
            nxt["delete"] = True
        if kind == "fin" or (kind in ("patch", "delete") and "finalizers" in self.keys and rng.random() < p["p_fin"]):
            atoms = [("fin", "other")]
            f = {}
            form = rng.choice(["add", "remove", "empty", "both"])
            if form in ("add", "both"):
                f["add"] = [{"value": v} for v in rng.sample(FIN_VALUES, rng.choice([1, 2]))]
            if form in ("remove", "both"):
                f["remove"] = [{"value": rng.choice(FIN_VALUES)}]
            if form == "empty":
                f["empty"] = True
            atoms += [("fin", x["value"]) for x in f.get("add", []) + f.get("remove", [])]
            if self.bits.fits(atoms):
                self.bits.take(atoms)
                nxt["finalizers"] = f
        for _ in range(n_any):
            exprs.append(self.requirement(multi_in=True))
        if pair is not None:
            exprs += self.same_key_pair(pair == "contradictory")
        for _ in range(rng.choice(p["extra_reqs"])):
            exprs.append(self.requirement())
        slots = 0  # any-clauses: a multi-value In, Exists on the finalizer set (KWK_MAX_ANY = 4)
        kept = []
        for r in exprs:
            uses = (r["operator"] == "In" and len(r["values"]) > 1) or (r["key"] == FINS and r["operator"] == "Exists")
            if uses and slots == 4:
                continue
            slots += uses
            kept.append(r)
        exprs = kept
        sel = {}
        if "labels" in self.keys and rng.random() < p["p_match_labels"]:
            k = rng.choice(sorted(LABELS))
            v = rng.choice(LABELS[k])
            if self.bits.fits([("lit", label_key(k), v)]):
                self.bits.take([("lit", label_key(k), v)])
                sel["matchLabels"] = {k: v}
        if "annotations" in self.keys and rng.random() < p["p_match_labels"]:
            k = rng.choice(sorted(ANNOTATIONS))
            v = rng.choice(ANNOTATIONS[k])
            if self.bits.fits([("lit", annotation_key(k), v)]):
                self.bits.take([("lit", annotation_key(k), v)])
                sel["matchAnnotations"] = {k: v}
        if not exprs and not sel:
            exprs.append(self.requirement())
        rng.shuffle(exprs)
        if exprs:
            sel["matchExpressions"] = exprs
        spec = {"resourceRef": {"apiGroup": API_GROUP, "kind": KIND}, "selector": sel, "next": nxt}
        self.getters(spec)
        if rng.random() < p["p_immediate"]:
            spec["immediateNextStage"] = True
        return {"apiVersion": "kwok.x-k8s.io/v1alpha1", "kind": "Stage", "metadata": {"name": "s%02d-%s" % (i, kind)},
                "spec": spec}

    def stages(self) -> List[dict]:
        rng, p = self.rng, self.p
        n = p["n_stages"]
        kinds = [rng.choice(p["kinds"]) for _ in range(n)]
        if p["loops"]:  # one bit per patch that may turn out idempotent
            self.bits.limit -= sum(k == "patch" for k in kinds)
            assert self.bits.limit >= 4, "max_bits leaves no room for selectors"
        n_any = [0] * n
        for j in range(min(n, p["any4_stages"])):
            n_any[j] = 4
        for j in range(p["any4_stages"], n):
            if rng.random() < p["p_multi_in"]:
                n_any[j] = rng.randint(1, 3)
        pairs: List[Optional[str]] = [None] * n
        for j in range(n):
            r = rng.random()
            if r < p["p_contradictory"]:
                pairs[j] = "contradictory"
            elif r < p["p_contradictory"] + p["p_pair"]:
                pairs[j] = "compatible"
        docs = [self.stage(j, kinds[j], n_any[j], pairs[j]) for j in range(n)]
        if p["fill_bits"]:  # literals no object carries, up to exactly max_bits feature bits
            extra = []
            while self.bits.used < self.bits.limit:
                v = "X%d" % len(extra)
                self.bits.take([("lit", PHASE, v)])
                extra.append(v)
            if extra:
                docs[-1]["spec"]["selector"].setdefault("matchExpressions", []).append(_req(PHASE, "NotIn", extra))
        if p["no_selector_stage"]:  # NewLifecycle drops it
            d = self.stage(n, "patch" if not p["loops"] else "none")
            d["metadata"]["name"] = "dropped-no-selector"
            del d["spec"]["selector"]
            docs.insert(rng.randrange(len(docs) + 1), d)
        return docs

    # -- objects
    def objects(self) -> List[dict]:
        rng, p = self.rng, self.p
        shapes = [{"size": 1}, {"size": 2, "parts": [{"name": "a"}]}, {"size": 3, "parts": [{"name": "a"}, {"name": "b"}]}]
        shapes = shapes[:p["n_classes"]]
        out = []
        for i in range(p["n_objs"]):
            md = {"name": "g%d" % i, "namespace": "default", "uid": "u%d" % i}
            lab = {k: rng.choice(vs) for k, vs in LABELS.items() if "labels" in self.keys and rng.random() < 0.6}
            ann = {k: rng.choice(vs) for k, vs in ANNOTATIONS.items() if "annotations" in self.keys and rng.random() < 0.6}
            if p["weights"] and rng.random() < p["p_ann"]:
                ann[W_ANN] = rng.choice(W_VALUES)
            if rng.random() < p["p_ann"]:
                ann[D_ANN] = rng.choice(D_VALUES)
            if p["jitter"] and rng.random() < p["p_ann"]:
                ann[J_ANN] = rng.choice(J_VALUES)
            if lab:
                md["labels"] = lab
            if ann:
                md["annotations"] = ann
            if "finalizers" in self.keys and rng.random() < 0.5:
                md["finalizers"] = rng.sample(FIN_VALUES + [FIN_UNKNOWN], rng.choice([1, 1, 2, 3]))
            if ("deletion" in self.keys or p["deletions"]) and rng.random() < 0.4:
                md["deletionTimestamp"] = rng.choice(DEL_VALUES)
            o = {"apiVersion": API_GROUP, "kind": KIND, "metadata": md, "spec": dict(rng.choice(shapes))}
            st = {}
            if rng.random() < 0.8:
                st["phase"] = rng.choice(self.phases)
            if "n" in self.keys and rng.random() < 0.6:
                st["n"] = rng.choice(NUMS)
            if p["loops"] and rng.random() < 0.5:
                st["note"] = rng.choice(["x", "y"])
            if st or rng.random() < 0.5:
                o["status"] = st
            out.append(o)
        return out


DEFAULTS = dict(
    n_stages=6, n_objs=300, loops=False, max_bits=32, fill_bits=False,
    keys=("phase", "n", "labels", "annotations", "deletion", "finalizers"), n_phases=4, n_classes=2,
    kinds=("patch", "patch", "patch", "delete", "fin", "none"), extra_reqs=(0, 1, 1, 2),
    weights=True, odd_weights=0.3, jitter=True, p_delay=0.4, p_from=0.35, p_ann=0.35, p_fin=0.2, p_immediate=0.15,
    p_multi_in=0.3, any4_stages=0, p_pair=0.2, p_contradictory=0.1, p_match_labels=0.25, no_selector_stage=False,
    deletions=True, p_guard=0.5, p_two_fields=0.35, chain=False,
)


def make_case(seed: int, **params) -> Tuple[List[dict], List[dict]]:
    p = dict(DEFAULTS)
    unknown = set(params) - set(p)
    assert not unknown, unknown
    p.update(params)
    g = _Gen(seed, p)
    docs = g.stages()
    return docs, g.objects()


# ---------------------------------------------------------------------------------------------
# The fixed corpus: (name, seed, params).  Names are the pytest ids; an entry is never re-seeded
# to make a failure go away.
_NARROW = dict(keys=("phase", "labels"), n_phases=3, weights=False, jitter=False, p_from=0.0, p_multi_in=0.0,
               p_pair=0.0, p_contradictory=0.0, p_match_labels=0.0, extra_reqs=(0, 0, 1), p_fin=0.0,
               kinds=("patch", "patch", "patch", "delete", "none"), deletions=False, p_immediate=0.0)
CORPUS = [
    # <= 16-bit words (pred + class + stage code + 5 flags): table-only, then delayed
    ("w16-table-a", 101, dict(_NARROW, n_stages=3, max_bits=8, p_delay=0.0, n_objs=300)),
    ("w16-table-b", 102, dict(_NARROW, n_stages=4, max_bits=7, p_delay=0.0, n_objs=320)),
    ("w16-5to8-stages", 103, dict(_NARROW, n_stages=6, max_bits=7, p_delay=0.0, n_objs=300)),
    ("w16-7-stages-delay", 104, dict(_NARROW, n_stages=7, max_bits=7, p_delay=0.5, n_objs=300)),
    ("w16-delay-a", 105, dict(_NARROW, n_stages=3, max_bits=8, p_delay=0.7, n_objs=300)),
    ("w16-delay-jitter", 106, dict(_NARROW, n_stages=4, max_bits=7, p_delay=0.8, jitter=True, weights=True,
                                   n_objs=300)),
    ("w16-contradictory", 107, dict(_NARROW, n_stages=4, max_bits=7, p_delay=0.3, p_contradictory=0.5, n_objs=300)),
    # at most one candidate per state and no getter expressions: the 1-byte dictionary ids
    # (32 ids per word class: few distinct (feature bits, class) pairs)
    ("b8-chain-4", 111, dict(_NARROW, chain=True, keys=("phase",), extra_reqs=(0,), n_stages=4, n_phases=4, max_bits=7,
                             p_delay=0.0, n_objs=320)),
    ("b8-chain-6", 112, dict(_NARROW, chain=True, keys=("phase",), extra_reqs=(0,), n_stages=6, n_phases=6, max_bits=7,
                             n_classes=1, p_delay=0.0, n_objs=320)),
    ("b8-chain-delay", 113, dict(_NARROW, chain=True, keys=("phase",), extra_reqs=(0,), n_stages=4, n_phases=4,
                                 max_bits=7, n_classes=1, p_delay=0.7, n_objs=320)),
    # 17-28 bit words: the fused 8-byte record
    ("w28-a", 201, dict(n_stages=5, max_bits=14, n_objs=400)),
    ("w28-b", 202, dict(n_stages=6, max_bits=16, n_objs=400, no_selector_stage=True)),
    ("w28-c", 203, dict(n_stages=8, max_bits=17, n_objs=400, p_contradictory=0.3)),
    ("w28-any4", 204, dict(n_stages=5, max_bits=18, n_objs=400, any4_stages=1)),
    ("w28-getters", 205, dict(n_stages=6, max_bits=16, n_objs=500, p_delay=0.8, p_from=0.7, p_ann=0.6,
                              odd_weights=0.6)),
    ("w28-overlap", 206, dict(n_stages=8, max_bits=12, n_objs=400, keys=("phase", "n", "finalizers"),
                              extra_reqs=(0,), p_multi_in=0.0, odd_weights=0.5)),
    ("w28-deletion", 207, dict(n_stages=6, max_bits=15, n_objs=400, p_delay=0.9, p_from=0.9,
                               keys=("phase", "deletion", "finalizers", "n"))),
    # 29-32 bit words: 4-byte words
    ("w32-a", 301, dict(n_stages=7, max_bits=21, fill_bits=True, n_objs=400, n_phases=6)),
    ("w32-b", 302, dict(n_stages=8, max_bits=22, fill_bits=True, n_objs=400, n_phases=5)),
    ("w32-c", 303, dict(n_stages=9, max_bits=22, fill_bits=True, n_objs=400, p_contradictory=0.25)),
    ("w32-d", 304, dict(n_stages=12, max_bits=21, fill_bits=True, n_objs=400, keys=("phase", "n", "deletion"))),
    # wider than 32 bits: the 8-byte state
    ("wide-a", 401, dict(n_stages=8, max_bits=30, fill_bits=True, n_objs=400, n_phases=6)),
    ("wide-32bits", 402, dict(n_stages=10, max_bits=32, fill_bits=True, n_objs=400, n_phases=6)),
    # many stages over a narrow key vocabulary (exploration grows with reachable states)
    ("w28-32stages", 403, dict(n_stages=32, max_bits=16, n_objs=400, keys=("phase", "n"), n_phases=4,
                                extra_reqs=(0, 0, 1), p_multi_in=0.1)),
    ("w28-20stages", 404, dict(n_stages=20, max_bits=14, n_objs=400, keys=("phase", "finalizers"), n_phases=4,
                                extra_reqs=(0, 1))),
    # idempotent patches: applied bits, re-match suppression, delta conflicts
    ("loops-a", 501, dict(loops=True, n_stages=5, max_bits=18, n_objs=300)),
    ("loops-b", 502, dict(loops=True, n_stages=6, max_bits=20, n_objs=300, p_delay=0.6)),
    ("loops-c", 503, dict(loops=True, n_stages=8, max_bits=24, n_objs=300, keys=("phase", "n", "labels"))),
    ("loops-12stages", 504, dict(loops=True, n_stages=12, max_bits=26, n_objs=300, keys=("phase", "n"),
                                 kinds=("patch", "patch", "patch", "patch", "delete", "none"), extra_reqs=(0, 1),
                                 p_guard=0.15, p_two_fields=0.6)),
    ("loops-narrow16", 505, dict(_NARROW, loops=True, n_stages=3, max_bits=8, p_delay=0.3, n_objs=300)),
    ("loops-d", 506, dict(loops=True, n_stages=7, max_bits=22, n_objs=300, p_contradictory=0.3)),
    ("loops-e", 507, dict(loops=True, n_stages=10, max_bits=28, n_objs=300, keys=("phase", "n", "finalizers"),
                          kinds=("patch", "patch", "fin", "delete", "none"))),
    ("loops-applied", 509, dict(loops=True, n_stages=12, max_bits=30, n_objs=300, keys=("phase",), n_phases=3,
                                kinds=("patch", "patch", "none"), extra_reqs=(0,), p_guard=0.0, p_pair=0.0,
                                p_contradictory=0.0, p_multi_in=0.0, p_match_labels=0.0, p_two_fields=0.2)),
    # exactly four idempotent stages, one past index 8: a Python set iterates them out of order
    ("loops-4applied", 558, dict(loops=True, n_stages=12, max_bits=30, n_objs=300, keys=("phase", "labels"), n_phases=3,
                                 kinds=("patch", "none", "none", "delete"), extra_reqs=(0, 1), p_guard=0.1, p_pair=0.0,
                                 p_contradictory=0.0, p_multi_in=0.0, p_match_labels=0.0, p_two_fields=0.3)),
    ("loops-f", 508, dict(loops=True, n_stages=6, max_bits=16, n_objs=300, keys=("phase", "n", "deletion"),
                          p_delay=0.7, p_from=0.6)),
]
CASE_IDS = [c[0] for c in CORPUS]
LOOPS = {c[0]: bool(c[2].get("loops")) for c in CORPUS}


@functools.lru_cache(maxsize=None)
def case(name: str):
    _, seed, params = next(c for c in CORPUS if c[0] == name)
    return make_case(seed, **params)


def run_params(name: str) -> dict:
    """kind_salt / slot_base of a case's runs: non-zero for every third case."""
    i = CASE_IDS.index(name)
    return {"kind_salt": 3, "slot_base": 1 << 33} if i % 3 == 1 else {"kind_salt": 0, "slot_base": 0}


class Step:
    """The oracle's state after one step (what parity_util.compare_state reads of an OracleSim)."""
    __slots__ = ("fired", "objs", "pending", "due", "dirty", "matcherr", "deletion")


class OracleRun:
    """One OracleSim run over NOWS, kept step by step; and what the coverage conditions need,
    computed with the oracle's own matcher and getters (refcpu)."""

    def __init__(self, docs, objs, slots=None, kind_salt=0, slot_base=0, nows=NOWS, harness=False):
        import copy
        from oracle import refcpu
        from oracle.sim import OracleSim
        sim = OracleSim(docs, objs, slots=slots, kind_salt=kind_salt, slot_base=slot_base, harness=harness)
        snap = copy.deepcopy if harness else list  # the harness stamps deletionTimestamps in place
        self.sim, self.names, self.slots = sim, sim.names, sim.slots
        self.docs = [d for d in docs if (d.get("spec") or {}).get("selector") is not None]
        self.steps: List[Step] = []
        self.seen = set()
        memo = {}
        for k, now in enumerate(nows):
            before = snap(sim.objs)
            was_dirty = list(sim.dirty)
            fired = sim.step(now, RUN_SEED, k)
            st = Step()
            st.fired = sorted(fired)
            st.objs, st.pending, st.due = snap(sim.objs), list(sim.pending), list(sim.due)
            st.dirty, st.matcherr = list(sim.dirty), list(sim.matcherr)
            st.deletion = [sim.deletion_s(i) for i in range(len(sim.objs))]
            self.steps.append(st)
            if any(st.matcherr):
                self.seen.add("matcherr")
            pos = {s: i for i, s in enumerate(sim.slots)}
            fired_at = {pos[s]: (stage, fl) for s, stage, fl in fired}
            for i, (stage, fl) in fired_at.items():
                self.seen.add("delete" if fl & 1 else ("rematch" if fl & 2 else "no-rematch"))
                a, b = before[i], sim.objs[i]
                if a is not None and b is not None and (a.get("metadata") or {}).get("finalizers") != (b.get("metadata") or {}).get("finalizers"):
                    self.seen.add("finalizers-changed")
            for i, o in enumerate(before):  # the objects matched in this step
                if o is None or not was_dirty[i]:
                    continue
                key = (json.dumps({k2: v for k2, v in o.items() if k2 != "metadata"}, sort_keys=True),
                       json.dumps({k2: v for k2, v in o["metadata"].items() if k2 not in ("name", "uid")}, sort_keys=True))
                cands = memo.get(key)
                if cands is None:
                    m = sim.lc.match_mask(o)
                    cands = memo[key] = [(s, sim.lc.weight(s, o)) for s in range(len(self.names)) if m >> s & 1]
                if len(cands) >= 2:
                    if sum(1 for _, (w, ok) in cands if ok and w > 0) >= 3:
                        self.seen.add("3-positive-weights")
                    if all(ok and w == 0 for _, (w, ok) in cands):
                        self.seen.add("all-weights-0")
                picked, _ = sim.lc.match(o, now, RUN_SEED ^ (kind_salt << 32), k, slot_base + sim.slots[i])
                if picked is None or picked < 0:
                    continue
                d = (self.docs[picked]["spec"].get("delay"))
                if d is None:
                    continue
                src = (d.get("durationFrom") or {}).get("expressionFrom")
                dv, _ = refcpu.duration_from(None if d.get("durationMilliseconds") is None else
                                             d["durationMilliseconds"] * 10**6, src, o, now)
                if src is not None:
                    res = refcpu.query(src, o) or []
                    ts = refcpu.parse_rfc3339(res[0]) if res and isinstance(res[0], str) and res[0] else None
                    if ts is not None:
                        self.seen.add("abs-past" if ts[0] * 10**9 + ts[1] <= now else "abs-future")
                        if src == DELETION:
                            self.seen.add("deletion-column")
                if "jitterDurationMilliseconds" in d or "jitterDurationFrom" in d:
                    jsrc = (d.get("jitterDurationFrom") or {}).get("expressionFrom")
                    jms = d.get("jitterDurationMilliseconds")
                    jv, jok = refcpu.duration_from(None if jms is None else jms * 10**6, jsrc, o, now)
                    if jok and jv > dv:
                        self.seen.add("jitter-draw")
        self.total = sum(len(s.fired) for s in self.steps)
        self.per_stage = [0] * len(self.names)
        for s in self.steps:
            for _, stage, _ in s.fired:
                self.per_stage[stage] += 1


# cases that also run with the churn harness (HarnessSpec: .status.phase Failed is terminal; the
# harness deletes terminal objects and re-creates deleted ones from their spec)
HARNESS_CASES = ("b8-chain-4", "w28-getters", "w32-a")


@functools.lru_cache(maxsize=None)
def oracle_run(name: str, harness: bool = False) -> OracleRun:
    docs, objs = case(name)
    return OracleRun(docs, objs, harness=harness, **run_params(name))


def word_bits(prog) -> int:
    """The packed state word of a compiled program (make_fmt in engine.hip, as
    parity_util.expected_state_bytes): pred | class | stage code | 5 flags."""
    t = prog.table()
    return (t.pred_bits or 32) + max(0, t.n_classes - 1).bit_length() + t.n_stages.bit_length() + 5


def has_delay(docs) -> bool:
    return any((d["spec"].get("delay") is not None) for d in docs if d["spec"].get("selector") is not None)


def compile_python(docs, objs, harness=False):
    from kwok_amd.host.compiler import HarnessSpec, KindProgram
    from kwok_amd.host.stages import stage_from_v1alpha1
    kp = KindProgram([stage_from_v1alpha1(d) for d in docs], HarnessSpec() if harness else None)
    kp.explore(objs)
    return kp


def compile_native(docs, objs, harness=False):
    from kwok_amd.host.compiler import HarnessSpec
    from kwok_amd.host.native_compiler import NativeProgram
    nat = NativeProgram(docs, HarnessSpec() if harness else None)
    nat.explore(objs)
    return nat


def state_key(o) -> str:
    """An object's state without its identity (name, uid): equal keys, equal features."""
    md = {k: v for k, v in o["metadata"].items() if k not in ("name", "uid")}
    return json.dumps([md, o.get("spec"), o.get("status", "-")], sort_keys=True)


def expected_rows(run: OracleRun, desc: dict):
    """Per step, the device rows the oracle's state implies, as arrays over the run's objects
    (what parity_util.compare_state checks, vectorised): alive, pending stage (0xFF none), due,
    feature bits by the oracle's jq (without the applied bits), deletion column, dirty flag."""
    import numpy as np
    from oracle.sim import oracle_pred
    memo = {}
    out = []
    for st in run.steps:
        n = len(st.objs)
        alive = np.array([o is not None for o in st.objs], dtype=bool)
        stage = np.array([0xFF if p is None else p for p in st.pending], dtype=np.int64)
        due = np.array(st.due, dtype=np.int64)
        pred = np.zeros(n, dtype=np.int64)
        for i, o in enumerate(st.objs):
            if o is not None:
                k = state_key(o)
                if k not in memo:
                    memo[k] = oracle_pred(desc, o)
                pred[i] = memo[k]
        dels = np.array(st.deletion, dtype=np.int64)
        dirty = np.array(st.dirty, dtype=bool)
        out.append((alive, stage, due, pred, dels, dirty))
    return out
