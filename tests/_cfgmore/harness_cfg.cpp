// tests/_cfgmore/harness_cfg.cpp — TEST-ONLY: tests/_gen/harness.cpp (generated code against the interpreter, state by state and slot by
// slot) with the interpreter that knows the cfg's ACTION_CONSTRAINTs and VIEW (spec_vm_cfg.h: SpecVmCfg, what the engine runs for a
// compiled program) in the place of SpecVm.  Built per program by tests/cfgmore.py gen_check.
#include GEN_HEADER
#include "spec_vm_cfg.h"
#define SpecVm SpecVmCfg
#include "../_gen/harness.cpp"
