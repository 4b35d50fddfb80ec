------------------------------ MODULE leave_enabled_unfair ------------------------------
(* The twin of leave_enabled without `fair`: nobody has to take the step out, the two-state cycle is a fair component of the ~Q subgraph (no process is fair) and  (q = 0) ~> (q = 1)  is VIOLATED. *)
EXTENDS Naturals

(* --algorithm leave_enabled_unfair
variables x = 0, q = 0;

process Spin = 0
begin
  S: while q = 0 do
       x := 1 - x;
     end while;
end process

process Leave = 1
begin
  L: q := 1;
end process

end algorithm *)

Reaches == (q = 0) ~> (q = 1)
=============================================================================
