------------------------------- MODULE unlogged -------------------------------
(* For mc_engine_behaviours with MC_BEH_F_HIDDEN (`mc -behaviours FILE -hidden H`): a process that takes two internal labels between
   two writes of the logged variable.  An implementation that logs x when it changes records x = 0, 1, 3; the model reaches x = 3 from
   x = 1 through b and c, which move only t and pc.  Without -hidden the log is rejected at observation 3 (the only step from x = 1
   leaves x = 1); with -hidden 1 still (two steps are missing); with -hidden 2 it is accepted.
   With Leaky = TRUE (unlogged_leaky.cfg) the internal label c does touch x (x = 2, which the log does not have): a step that changes an
   observed cell is no hidden step, and the log stays rejected whatever H is. *)
EXTENDS Naturals
CONSTANT Leaky
(* --algorithm unlogged
variables x = 0, t = 0;

process P = 0
begin
  a: x := 1;
  b: t := x + 1;
  c: if Leaky then
       x := t;
     else
       t := t + 1;
     end if;
  d: x := 3;
end process

end algorithm *)
=============================================================================
