------------------------------- MODULE diamond -------------------------------
(* For mc_engine_behaviours: two candidates converge.  h starts as 1 or 2 and is not logged; the only step forgets it.  Logging x: K_0 has
   two members, both lead to the one row (h = 0, x = 1): peak 2, candidates 1. *)
EXTENDS Naturals
(* --algorithm diamond
variables h \in 1..2, x = 0;

process P = 0
begin
  s: h := 0;
     x := 1;
end process

end algorithm *)
=============================================================================
