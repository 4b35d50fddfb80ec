---------------------------- MODULE failing_step -----------------------------
(* For mc_engine_behaviours: a step whose Assert fails is no step.  The log x = 0, 1, 2 matches the assignments, but the spec's second
   step asserts x = 0 first: the only successor that could match observation 2 is an error (errors = 1), and the behaviour is
   rejected there. *)
EXTENDS Naturals, TLC
(* --algorithm failing_step
variables x = 0;

process P = 0
begin
  a: x := 1;
  b: assert x = 0;
     x := 2;
end process

end algorithm *)
=============================================================================
