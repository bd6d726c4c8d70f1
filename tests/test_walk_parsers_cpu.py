"""No GPU: the command lines of python -m agdiff_amd.medoids, .pam, .silhouette and .picks as data -- every option with its
default, `required`, choices, type, nargs, metavar and help text, in the order --help prints them, and the message with which each
shared misuse exits.  The four parsers are put together from shared pieces (agdiff_amd.ensemble); this is the record they are held to."""
import pytest

# (option, default, required, choices, type, nargs, metavar, help)
SHARED = [
    ("--samples", None, True, None, None, None, None, None),
    ("--testset", None, True, None, None, None, None, None),
    ("--out", None, True, None, None, None, None, None),
    ("--device", "cuda", False, None, None, None, None, None),
    ("--align", False, False, None, None, 0, None, "superpose the conformers that are written on the first of them"),
    ("--fix-handedness", False, False, None, None, 0, None, "invert the mirror-image conformers first (needs stereo_<i> in --testset)"),
    ("--fix-double-bonds", False, False, None, None, 0, None,
     "turn over the double bonds of the wrong E/Z parity first, after --fix-handedness (needs ez_quads_<i> and ez_<i> in --testset: "
     "python -m agdiff_amd.ezbonds); also writes ez_state_<i> [G, D].  --drop-invalid and --drop-bent judge the conformers as sampled, "
     "before the flip, which can bring the two sides of a bond into contact: the driver's order (flip, repair, check) is the one to "
     "use when that matters"),
    ("--drop-invalid", False, False, None, None, 0, None,
     "leave the conformers with a bond out of bounds or a steric clash (agdiff_amd.validity) out; also writes valid_<i> [G]"),
    ("--drop-bent", False, False, None, None, 0, None,
     "leave the conformers with an aromatic ring or a double bond out of plane (agdiff_amd.planarity) out; also writes flat_<i> [G]"),
]
TFD = [
    ("--tfd", False, False, None, None, 0, None, "the torsion fingerprint deviation (agdiff_amd.torsions) in the RMSD's place"),
    ("--tfd-rings", False, False, None, None, 0, None,
     "with --tfd: the rings are terms of the TFD too (agdiff_amd.rings): chair and boat are far apart"),
]
COUNT = [("--count", None, True, None, "int", None, None, "the number of medoids per molecule")]
OPTIONS = {
    "medoids": SHARED + COUNT + TFD + [
        ("--init", "maxmin", False, ("maxmin", "first"), None, None, None,
         "the seeds: the first K MaxMin picks (agdiff_amd.picks), or the first K conformers that are not left out"),
        ("--max-iter", 32, False, None, "int", None, None, "at most this many updates (1 .. 128)"),
    ],
    "pam": SHARED + COUNT + TFD + [
        ("--init", "build", False, ("build", "maxmin", "first", "alternate"), None, None, None,
         "where the swaps start: PAM's BUILD, the first K MaxMin picks, the first K conformers that are not left out, or what python -m "
         "agdiff_amd.medoids ends at from MaxMin seeds"),
        ("--max-swaps", 4096, False, None, "int", None, None, "at most this many exchanges (0: the seeds' assignment)"),
    ],
    "silhouette": SHARED + [
        ("--labels", None, False, None, None, None, None,
         "an .npz with one integer array per molecule, `<label-key>_<i>` [G]: the clustering to score (what python -m agdiff_amd.clusters / "
         ".medoids / .ensemble / .picks wrote)"),
        ("--label-key", "cluster", False, None, None, None, None,
         "the key of --labels: cluster (default), or owner for python -m agdiff_amd.picks"),
        ("--sweep", None, False, None, "int", 2, ("LO", "HI"),
         "no labels: run k-medoids for K = LO .. HI and keep the K with the highest mean silhouette"),
    ] + TFD + [
        ("--init", "maxmin", False, ("maxmin", "first"), None, None, None, "with --sweep: k-medoids' seeds (agdiff_amd.medoids)"),
        ("--max-iter", 32, False, None, "int", None, None, "with --sweep: at most this many updates per K (1 .. 128)"),
    ],
    "picks": SHARED + [
        ("--count", None, False, None, "int", None, None, "pick at most this many conformers per molecule"),
        ("--radius", None, False, None, "float", None, None,
         "stop once every conformer is within this distance of a pick (Angstrom of heavy-atom RMSD; with --tfd a TFD in [0, 1]); with "
         "--count, whichever comes first"),
    ] + TFD + [
        ("--first", None, False, None, "int", None, None, "the conformer picked first (default: the first one that is not left out)"),
    ],
}

BASE = ["--samples", "s.npz", "--testset", "t.npz", "--out", "o.npz"]
# (module, the arguments after BASE, the message after "error: ")
MISUSES = [
    ("medoids", ["--count", "3", "--tfd-rings"], "--tfd-rings goes with --tfd"),
    ("medoids", ["--count", "0"], "--count must be at least 1"),
    ("medoids", ["--count", "3", "--max-iter", "0"], "--max-iter must be in 1 .. 128"),
    ("medoids", ["--count", "3", "--max-iter", "129"], "--max-iter must be in 1 .. 128"),
    ("pam", ["--count", "3", "--tfd-rings"], "--tfd-rings goes with --tfd"),
    ("pam", ["--count", "0"], "--count must be at least 1"),
    ("pam", ["--count", "3", "--max-swaps", "-1"], "--max-swaps must be at least 0"),
    ("silhouette", ["--sweep", "2", "4", "--tfd-rings"], "--tfd-rings goes with --tfd"),
    ("silhouette", ["--labels", "l.npz", "--tfd-rings"], "--tfd-rings goes with --tfd"),
    ("silhouette", ["--sweep", "2", "4", "--max-iter", "0"], "--max-iter must be in 1 .. 128"),
    ("silhouette", ["--sweep", "2", "4", "--max-iter", "129"], "--max-iter must be in 1 .. 128"),
    ("silhouette", ["--sweep", "1", "4"], "--sweep LO HI needs 2 <= LO <= HI"),
    ("silhouette", ["--sweep", "5", "4"], "--sweep LO HI needs 2 <= LO <= HI"),
    ("silhouette", ["--sweep", "2", "66"], "--sweep runs at most 64 values of K"),
    ("silhouette", [], "exactly one of --labels and --sweep"),
    ("silhouette", ["--labels", "l.npz", "--sweep", "2", "4"], "exactly one of --labels and --sweep"),
    ("picks", ["--count", "3", "--tfd-rings"], "--tfd-rings goes with --tfd"),
    ("picks", [], "at least one of --count and --radius is required"),
]


def _module(name):
    import importlib
    return importlib.import_module("agdiff_amd." + name)


@pytest.mark.parametrize("name", sorted(OPTIONS))
def test_every_option_is_what_it_was(name):
    module = _module(name)
    ap = module._parser()
    got = [(a.option_strings, a.default, a.required, None if a.choices is None else tuple(a.choices),
            None if a.type is None else a.type.__name__, a.nargs, a.metavar, a.help)
           for a in ap._actions if a.option_strings != ["-h", "--help"]]
    want = [([row[0]],) + row[1:] for row in OPTIONS[name]]
    assert [g[0] for g in got] == [w[0] for w in want]
    for g, w in zip(got, want):
        assert g == w, g[0]
    assert ap.description == module.main.__doc__ and ap.description.startswith("python -m agdiff_amd.%s " % name)


@pytest.mark.parametrize("name, extra, message", MISUSES)
def test_every_misuse_exits_with_its_message(name, extra, message, capsys):
    ap = _module(name)._parser()
    with pytest.raises(SystemExit) as e:
        ap.parse_args(BASE + extra)
    assert e.value.code == 2
    assert capsys.readouterr().err.rstrip().endswith("error: " + message)


def test_the_flags_go_with_tfd_when_it_is_given():
    for name, extra in (("medoids", ["--count", "3"]), ("pam", ["--count", "3"]), ("silhouette", ["--sweep", "2", "4"]),
                        ("picks", ["--count", "3"])):
        ap = _module(name)._parser()
        a = ap.parse_args(BASE + extra)
        assert a.tfd is False and a.tfd_rings is False
        a = ap.parse_args(BASE + extra + ["--tfd"])
        assert a.tfd is True and a.tfd_rings is False
        a = ap.parse_args(BASE + extra + ["--tfd", "--tfd-rings"])
        assert a.tfd is True and a.tfd_rings is True
