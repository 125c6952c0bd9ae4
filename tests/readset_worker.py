"""The child process of the read-set tests, and the parent's side of it (run_report).

A test that looks at cigar digests needs a process of its own (ABPOA_HIP_CIGAR_DIGEST is read once per process), and so does one that reads what the library
says on stderr.  The parent starts `python tests/readset_worker.py <jobs-module> [<selector>]`; the jobs come from the test module itself:
`<jobs-module>.make_jobs(*selector)` returns {job: spec}, a spec being a dict of

  params           Params keywords, or a Params
  sets             the read-sets
  forms            {form: environment of that device run}, run in this order
  env              environment of every device run of the job, beside the form's own                                  (default: none)
  first_set_forms  forms that run sets[:1] only                                                                       (default: none)
  record           optional fields of a device run, of OPTIONAL below                                                 (default: none)
  ref_record       optional fields of the reference run                                                               (default: none)
  n_threads        host threads of a device run (default 4), ref_threads: of the reference run (default 4)
  ref_first        the reference run comes before the forms, not after them                                           (default: after)
  env_seen         names of environment variables whose values, as a run finds them, go into its record as `env`      (default: none)

Every job runs through api.msa_batch once per form on the device and once, keyed `ref`, through the CPU build of the host layer whose aligner is the plain-C
oracle (tests/cpu_shim.cpp).  A run's record always has status, cons and cov per set; MSA rows are asked of a run exactly when it records `msa`.  A form's
variables are set before its run and removed after it.  Before each device run the line `[job] <job> <form>` goes to stderr, flushed, so that the parent can
tell the library's messages apart; at the end one line `REPORT <json>` of {job: {form: record, "ref": record}} goes to stdout."""
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTIONAL = ("n_cells",            # DP cells per set
            "msa",                # MSA rows per set
            "dig",                # cigar digest per set (gpu_harness.cigar_digests)
            "last",               # result record of each set's last alignment (gpu_harness.last_alignments)
            "rounds_launches",    # launches of the all-rounds kernel during the run (the statistics are reset before it)
            "launches",           # row-kernel launches during the run (gpu_harness.row_launches)
            "n_host_sets",        # sets the run handed to the host driver
            "host_reasons")       # ... and why
# for tests/test_gpu_harness.py only: the CPU shim stands in for the device library, so that the protocol can be tested without a GPU
SHIM_AS_DEVICE = "READSET_WORKER_SHIM_AS_DEVICE"


def _run(lib, sets, p, n_threads, fields, env_seen):
    from abpoa_amd import api, ffi
    import gpu_harness as G
    assert set(fields) <= set(OPTIONAL), fields
    if "rounds_launches" in fields:
        lib.abpoa_hip_reset_stats()
    if "launches" in fields:
        G.row_launches(lib)
    res = api.msa_batch(sets, p, out_msa="msa" in fields, n_threads=n_threads, lib=lib)
    rec = dict(status=[r.status for r in res], cons=[r.cons_seq for r in res], cov=[list(map(int, r.cons_cov)) for r in res])
    if "launches" in fields:
        rec["launches"] = G.row_launches(lib)
    if "n_cells" in fields:
        rec["n_cells"] = [int(r.n_cells) for r in res]
    if "msa" in fields:
        rec["msa"] = [list(r.msa_seq) for r in res]
    if "dig" in fields:
        rec["dig"] = G.cigar_digests(lib, sets, p.m)
    if "last" in fields:
        rec["last"] = G.last_alignments(lib, sets, p.m)
    if "rounds_launches" in fields:
        rec["rounds_launches"] = int(ffi.stats()["rounds_launches"])
    if "n_host_sets" in fields:
        rec["n_host_sets"] = int(api.msa_timing(lib)["n_host_sets"])
    if "host_reasons" in fields:
        rec["host_reasons"] = api.host_reasons(lib)
    if env_seen:
        rec["env"] = {k: os.environ.get(k) for k in env_seen}
    return rec


def main(argv):
    sys.path.insert(0, ROOT)
    import helpers as H
    from abpoa_amd import api, ffi
    jobs = importlib.import_module(argv[0]).make_jobs(*argv[1:])
    shim = H.cpu_shim_lib()
    if os.environ.get(SHIM_AS_DEVICE):
        dev = shim
    else:
        dev = ffi.lib()
        ffi.check(dev.abpoa_hip_init(0))
    report = {}
    for job, spec in jobs.items():
        p = spec["params"] if isinstance(spec["params"], api.Params) else api.Params(**spec["params"])
        sets, seen = spec["sets"], spec.get("env_seen", ())
        rep = {}
        if spec.get("ref_first"):
            rep["ref"] = _run(shim, sets, p, spec.get("ref_threads", 4), spec.get("ref_record", ()), seen)
        for form, form_env in spec["forms"].items():
            env = dict(spec.get("env", {}), **form_env)
            os.environ.update(env)
            sys.stderr.write("[job] %s %s\n" % (job, form))
            sys.stderr.flush()
            rep[form] = _run(dev, sets[:1] if form in spec.get("first_set_forms", ()) else sets, p, spec.get("n_threads", 4), spec.get("record", ()), seen)
            for k in env:
                del os.environ[k]
        if not spec.get("ref_first"):
            rep["ref"] = _run(shim, sets, p, spec.get("ref_threads", 4), spec.get("ref_record", ()), seen)
        report[job] = rep
    print("REPORT " + json.dumps(report))


def run_report(jobs_module, selector=None, *, set_env, clear_env, timeout, want_log=False):
    """Parent side: one child for `jobs_module` (and `selector`), its environment this process's with `set_env` set and then every name of `clear_env` removed
    (each file lists exactly the switches its forms toggle).  Returns the report, and with want_log also {(job, form): what the library wrote to stderr during
    that run}.  A child that fails or reports nothing fails the assertion here, with the ends of its stdout and stderr in the message."""
    env = dict(os.environ, **set_env)
    for k in clear_env:
        env.pop(k, None)
    cmd = [sys.executable, os.path.abspath(__file__), jobs_module] + ([] if selector is None else [selector])
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=timeout)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("REPORT ")]
    assert r.returncode == 0 and lines, (r.stdout[-1500:], r.stderr[-3000:])
    report = json.loads(lines[0][7:])
    return (report, split_log(r.stderr)) if want_log else report


def split_log(stderr):
    """{(job, form): the lines between that run's `[job] <job> <form>` marker and the next}"""
    log, key = {}, None
    for ln in stderr.splitlines():
        if ln.startswith("[job] "):
            key = tuple(ln.split()[1:3])
            log[key] = []
        elif key:
            log[key].append(ln)
    return {k: "\n".join(v) for k, v in log.items()}


if __name__ == "__main__":
    main(sys.argv[1:])
