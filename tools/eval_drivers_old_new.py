"""What `cnn eval`, `evalnoise` and `evalrand` print and write, of two trees compared byte for byte (diagnostic;
profiles/r45_a_eval_drivers_old_new.txt). No device: the commands run under the stub context of tests/eval_stub.py, over its
corpus in a temporary folder, for every case of its matrix (the three commands x the option sets, hop 160 without and with
accuracy='centre'; none and segments at hop None as well).
    python tools/eval_drivers_old_new.py run OUT.json          per case: the sha256 of stdout (the temporary root and the run time
                                          replaced by fixed words), of its sorted lines, of every .npz member - named by its
                                          position as well, so that a reordered archive shows - and of every PNG
    python tools/eval_drivers_old_new.py compare OLD.json NEW.json    the table "case: identical / differs", and what differs
Run it in a checkout of each tree (this file and tests/eval_stub.py copied into the older one)."""
import hashlib, json, os, re, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def sha(data):
    return hashlib.sha256(data).hexdigest()[:16]


def run(out):
    import numpy as np
    import eval_stub
    res = {}
    with tempfile.TemporaryDirectory() as root:
        files = eval_stub.build_corpus(root)
        for command in eval_stub.COMMANDS:
            for name, accuracy, hop in eval_stub.MATRIX:
                case = "{} {}, hop {}, accuracy {}".format(command, name, hop, accuracy)
                entry = res[case] = {}
                for call in eval_stub.run_command(root, command, eval_stub.OPTION_SETS[name], accuracy, hop, files):
                    tag = "" if command == "evalrand" else call["files"][0] + ": "
                    text = re.sub(r"Total time: .*", "Total time: T", call["stdout"].replace(root, "ROOT"))
                    entry[tag + "stdout"] = sha(text.encode())
                    entry[tag + "stdout, sorted lines"] = sha("\n".join(sorted(text.splitlines())).encode())
                    entry[tag + "error"] = call["error"]
                    entry[tag + "device calls"] = sha(repr(call["log"]).encode())
                    for path, members in call["npz"].items():
                        entry[path + ": members in order"] = list(members)
                        for key, value in members.items():
                            entry[path + ": " + key] = sha(str(value.dtype).encode() + repr(value.shape).encode() + np.ascontiguousarray(value).tobytes())
                    for path, data in call["png"].items():
                        entry[path] = sha(data)
            print(command, "done", flush=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def compare(old, new):
    old, new = json.load(open(old)), json.load(open(new))
    for case in sorted(set(old) | set(new), key=lambda c: (list(old) + list(new)).index(c)):
        a, b = old.get(case, {}), new.get(case, {})
        differing = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
        print("{}: {}".format(case, "identical" if not differing else "differs in " + "; ".join(differing)))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        compare(sys.argv[2], sys.argv[3])
    else:
        raise SystemExit(__doc__)
